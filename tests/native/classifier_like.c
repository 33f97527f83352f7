/* A caller written the way the reference's predict_classifier drives a hierarchical classifier (classifier.c:707-726:
 * network_predict, hierarchy_predictions(predictions, net.outputs, net.hierarchy, 0), top_k over net.outputs), compiled
 * against include/ with the reference's own header names and linked to libsr_yolo2.so.  Prints one line per top entry
 * for the test to compare; then the leaves-only form of validate_classifier_single (classifier.c:514-520) after an
 * optional change_leaves, and one get_hierarchy_probability.
 *
 *   classifier_like <cfg> <weights> <frame.bin: c h w int32 header + CHW float32> <top> [leaf list]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "network.h"
#include "parser.h"
#include "cuda.h"
#include "utils.h"
#include "image.h"
#include "tree.h"

int main(int argc, char **argv)
{
    if (argc < 5) { fprintf(stderr, "usage: classifier_like cfg weights frame.bin top [leaf list]\n"); return 2; }
    cuda_set_device(0);
    network net = parse_network_cfg(argv[1]);
    load_weights(&net, argv[2]);
    set_batch_network(&net, 1);

    FILE *f = fopen(argv[3], "rb");
    int hdr[3];
    if (!f || fread(hdr, sizeof(int), 3, f) != 3) { fprintf(stderr, "bad frame file\n"); return 2; }
    image im = make_image(hdr[2], hdr[1], hdr[0]);
    if (fread(im.data, sizeof(float), (size_t)im.w * im.h * im.c, f) != (size_t)im.w * im.h * im.c) return 2;
    fclose(f);

    int top = atoi(argv[4]), i;
    int *indexes = calloc(top, sizeof(int));
    float *predictions = network_predict(net, im.data);
    float first = net.hierarchy ? get_hierarchy_probability(predictions, net.hierarchy, net.outputs - 1) : predictions[net.outputs - 1];
    if (net.hierarchy) hierarchy_predictions(predictions, net.outputs, net.hierarchy, 0);
    top_k(predictions, net.outputs, top, indexes);
    printf("OUTPUTS %d hierarchy %d\n", net.outputs, net.hierarchy ? net.hierarchy->n : 0);
    for (i = 0; i < top; ++i) printf("TOP %d %.9g\n", indexes[i], predictions[indexes[i]]);
    printf("LAST %.9g %.9g\n", first, predictions[net.outputs - 1]);

    if (net.hierarchy) {
        if (argc > 5) change_leaves(net.hierarchy, argv[5]);
        predictions = network_predict(net, im.data);
        hierarchy_predictions(predictions, net.outputs, net.hierarchy, 1);
        top_k(predictions, net.outputs, top, indexes);
        for (i = 0; i < top; ++i) printf("LEAF %d %.9g\n", indexes[i], predictions[indexes[i]]);
    }
    free(indexes);
    free_image(im);
    free_network(net);
    return 0;
}
