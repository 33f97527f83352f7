/* A drop-in user of the reference's optimize_picture, compiled against include/ with the reference's own header names: the
 * inner loop of run_nightmare (nightmare.c:258-278) without its file I/O.  nightmare.c has no header, so a caller declares
 * the function itself, with the reference's prototype, as darknet.c does for run_nightmare.
 *
 *   nightmare_like <cfg> <weights> <picture.bin> <w> <h> <max_layer> <iters> <out.bin>
 *       picture.bin: [3][h][w] floats; the picture after `iters` steps goes to out.bin. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "network.h"
#include "parser.h"
#include "image.h"
#include "cuda.h"

void optimize_picture(network *net, image orig, int max_layer, float scale, float rate, float thresh, int norm);

int main(int argc, char **argv)
{
    network net;
    image im;
    FILE *f;
    int n, iters, max_layer;
    if (argc != 9) { fprintf(stderr, "usage: nightmare_like cfg weights picture.bin w h max_layer iters out.bin\n"); return 2; }
    srand(0);
    cuda_set_device(0);
    net = parse_network_cfg(argv[1]);
    load_weights(&net, argv[2]);
    set_batch_network(&net, 1);
    im = make_image(atoi(argv[4]), atoi(argv[5]), 3);
    f = fopen(argv[3], "rb");
    if (!f || fread(im.data, sizeof(float), (size_t)im.w * im.h * im.c, f) != (size_t)im.w * im.h * im.c) { fprintf(stderr, "nightmare_like: cannot read %s\n", argv[3]); return 2; }
    fclose(f);
    max_layer = atoi(argv[6]);
    iters = atoi(argv[7]);
    for (n = 0; n < iters; ++n) {
        int layer = max_layer + rand() % 1 - 1 / 2;
        int octave = rand() % 4;
        optimize_picture(&net, im, layer, 1 / pow(1.33333333, octave), .04, 1., 1);
    }
    f = fopen(argv[8], "wb");
    if (!f) return 2;
    fwrite(im.data, sizeof(float), (size_t)im.w * im.h * im.c, f);
    fclose(f);
    free_image(im);
    free_network(net);
    return 0;
}
