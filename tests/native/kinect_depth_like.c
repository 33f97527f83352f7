/* The Kinect loop's per-frame sequence (KinectUtil_with_cam.cpp:1003-1118: drawDepth, two filtered hand crops and the
 * whole frame through the detector, caculateXYZinCameraSpace, objectBelong2Person) as the application would write it
 * against this library: y2_depth_upload + one test_detector_regions_depth, compiled against include/ with the
 * reference's own header names.  Prints one line per object for the test to compare with the Python path.
 *
 *   kinect_depth_like <cfg> <weights> <frame.u8: h w c int32 header + bytes>
 *                     <depth.bin: dh dw int32 header + uint16 depth + uint8 body + float map[H][W][2] + float table[dh][dw][2]>
 *                     <thresh> rx1 ry1 rw1 rh1 far1 rx2 ry2 rw2 rh2 far2
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>

#include "network.h"
#include "parser.h"
#include "cuda.h"
#include "utils.h"
#include "image.h"
#include "test_detector.h"

int main(int argc, char **argv)
{
    if (argc < 16) { fprintf(stderr, "usage: kinect_depth_like cfg weights frame.u8 depth.bin thresh (rx ry rw rh far) x 2\n"); return 2; }
    cuda_set_device(0);
    FILE *f = fopen(argv[3], "rb");
    int hdr[3], dhdr[2];
    if (!f || fread(hdr, sizeof(int), 3, f) != 3) { fprintf(stderr, "bad frame file\n"); return 2; }
    const int H = hdr[0], W = hdr[1], CH = hdr[2];
    unsigned char *frame = malloc((size_t)H * W * CH);
    if (fread(frame, 1, (size_t)H * W * CH, f) != (size_t)H * W * CH) return 2;
    fclose(f);
    f = fopen(argv[4], "rb");
    if (!f || fread(dhdr, sizeof(int), 2, f) != 2) { fprintf(stderr, "bad depth file\n"); return 2; }
    const int dh = dhdr[0], dw = dhdr[1];
    const size_t nd = (size_t)dh * dw, np = (size_t)H * W;
    uint16_t *depth = malloc(nd * 2);
    uint8_t *body = malloc(nd);
    float *map = malloc(np * 2 * sizeof(float)), *table = malloc(nd * 2 * sizeof(float));
    if (fread(depth, 2, nd, f) != nd || fread(body, 1, nd, f) != nd || fread(map, sizeof(float), np * 2, f) != np * 2 ||
        fread(table, sizeof(float), nd * 2, f) != nd * 2) { fprintf(stderr, "short depth file\n"); return 2; }
    fclose(f);
    const float thresh = (float)atof(argv[5]);

    y2_region items[3];
    float far_m[3] = {0, 0, 0};                                           /* the whole frame is not filtered */
    int i, j;
    for (i = 0; i < 3; ++i) {
        items[i].data = frame; items[i].h = H; items[i].w = W; items[i].c = CH; items[i].step = W * CH;
        items[i].x = items[i].y = items[i].rw = items[i].rh = 0;
    }
    for (i = 1; i < 3; ++i) {
        char **a = argv + 6 + 5 * (i - 1);
        items[i].x = atoi(a[0]); items[i].y = atoi(a[1]); items[i].rw = atoi(a[2]); items[i].rh = atoi(a[3]);
        far_m[i] = (float)atof(a[4]);                                     /* jointDistance + 0.3 */
    }

    network net = parse_network_cfg(argv[1]);
    load_weights(&net, argv[2]);
    set_batch_network(&net, 3);
    layer l = net.layers[net.n - 1];
    const int total = l.w * l.h * l.n;
    char **names = calloc(l.classes, sizeof(char *));
    for (i = 0; i < l.classes; ++i) { names[i] = malloc(32); snprintf(names[i], 32, "class%d", i); }

    if (y2_depth_set_camera_table(net, table, dh, dw) != 0) return 3;    /* once */
    y2_depth_frame df = { depth, body, map, dh, dw, H, W };               /* every frame */
    if (y2_depth_upload(net, &df) != 0) return 3;

    object *objs[3];
    int counts[3] = {0, 0, 0};
    for (i = 0; i < 3; ++i) objs[i] = calloc(total, sizeof(object));
    test_detector_regions_depth(names, net, items, 3, far_m, thresh, objs, counts);
    printf("COUNTS %d %d %d\n", counts[0], counts[1], counts[2]);
    for (i = 0; i < 3; ++i)
        for (j = 0; j < counts[i]; ++j) {
            const object *o = &objs[i][j];
            printf("OBJ %d %d %s %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %d %d\n", i, o->objClass, o->name, o->prob, o->x,
                   o->y, o->w, o->h, o->CameraX, o->CameraY, o->CameraZ, o->CameraWidth, o->CameraHeight, (int)o->flagBelong2Person,
                   o->bodyId);
        }
    free_network(net);
    return 0;
}
