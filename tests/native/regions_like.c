/* The Kinect loop's three detector calls per camera frame (the whole colour frame and two hand crops,
 * KinectUtil_with_cam.cpp:1029-1110) written both ways, compiled against include/ with the reference's own header
 * names: one test_detector_regions on a batch-3 network, and per item test_detector_img on a batch-1 network fed
 * the host-copied crop (BGR bytes -> RGB planes, v / 255., as ipl_to_image + rgbgr_image do), its boxes mapped into
 * the frame by y2_region_box_to_frame.  Prints one line per object for the test to compare.
 *
 *   regions_like <cfg> <weights> <frame.u8: h w c int32 header + bytes> <thresh> rx1 ry1 rw1 rh1 rx2 ry2 rw2 rh2
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "network.h"
#include "parser.h"
#include "cuda.h"
#include "utils.h"
#include "image.h"
#include "test_detector.h"

static void print_objects(const char *tag, int item, const object *o, int n)
{
    int i;
    for (i = 0; i < n; ++i)
        printf("%s %d %d %.9g %.9g %.9g %.9g %.9g %s %.9g %.9g %.9g\n", tag, item, o[i].objClass, o[i].prob, o[i].x, o[i].y,
               o[i].w, o[i].h, o[i].name, o[i].boxRGB[0], o[i].boxRGB[1], o[i].boxRGB[2]);
}

int main(int argc, char **argv)
{
    if (argc < 13) { fprintf(stderr, "usage: regions_like cfg weights frame.u8 thresh rx1 ry1 rw1 rh1 rx2 ry2 rw2 rh2\n"); return 2; }
    cuda_set_device(0);
    FILE *f = fopen(argv[3], "rb");
    int hdr[3];
    if (!f || fread(hdr, sizeof(int), 3, f) != 3) { fprintf(stderr, "bad frame file\n"); return 2; }
    const int H = hdr[0], W = hdr[1], CH = hdr[2];
    unsigned char *frame = malloc((size_t)H * W * CH);
    if (fread(frame, 1, (size_t)H * W * CH, f) != (size_t)H * W * CH) return 2;
    fclose(f);
    const float thresh = (float)atof(argv[4]);

    y2_region items[3];
    int i, k;
    for (i = 0; i < 3; ++i) {
        items[i].data = frame; items[i].h = H; items[i].w = W; items[i].c = CH; items[i].step = W * CH;
        items[i].x = items[i].y = items[i].rw = items[i].rh = 0;          /* item 0: the whole frame */
    }
    for (i = 1; i < 3; ++i) {
        items[i].x = atoi(argv[1 + 4 * i]); items[i].y = atoi(argv[2 + 4 * i]);
        items[i].rw = atoi(argv[3 + 4 * i]); items[i].rh = atoi(argv[4 + 4 * i]);
    }

    network net = parse_network_cfg(argv[1]);
    load_weights(&net, argv[2]);
    set_batch_network(&net, 3);
    layer l = net.layers[net.n - 1];
    const int total = l.w * l.h * l.n;
    char **names = calloc(l.classes, sizeof(char *));
    for (i = 0; i < l.classes; ++i) { names[i] = malloc(32); snprintf(names[i], 32, "class%d", i); }

    object *objs[3];
    int counts[3] = {0, 0, 0};
    for (i = 0; i < 3; ++i) objs[i] = calloc(total, sizeof(object));
    test_detector_regions(names, net, items, 3, thresh, objs, counts);
    printf("COUNTS %d %d %d\n", counts[0], counts[1], counts[2]);
    for (i = 0; i < 3; ++i) print_objects("REG", i, objs[i], counts[i]);

    network one = parse_network_cfg(argv[1]);
    load_weights(&one, argv[2]);
    set_batch_network(&one, 1);
    for (i = 0; i < 3; ++i) {
        const int rx = items[i].rw ? items[i].x : 0, ry = items[i].rw ? items[i].y : 0;
        const int rw = items[i].rw ? items[i].rw : W, rh = items[i].rw ? items[i].rh : H;
        image im = make_image(rw, rh, 3);
        int x, y, n = 0, j;
        for (k = 0; k < 3; ++k)
            for (y = 0; y < rh; ++y)
                for (x = 0; x < rw; ++x)
                    im.data[((size_t)k * rh + y) * rw + x] = (float)(frame[((size_t)(ry + y) * W + rx + x) * CH + (2 - k)] / 255.);
        object *crop = calloc(total, sizeof(object));
        test_detector_img(names, load_alphabet(), one, im, thresh, crop, &n);
        for (j = 0; j < n; ++j) y2_region_box_to_frame(&items[i], net.w, net.h, 0, &crop[j].x, &crop[j].y, &crop[j].w, &crop[j].h);
        print_objects("IMG", i, crop, n);
        free(crop);
        free_image(im);
    }
    free_network(one);
    free_network(net);
    return 0;
}
