/* The Grasp event of the Kinect loop (KinectUtil_with_cam.cpp:364-377 updateDepth -> desk_seg, :1508-1518) as the
 * application would write it against this library: camera table once, plane removal on, then per frame y2_depth_upload,
 * one test_detector_regions_depth in the Grasp event and the plane record.  Compiled against include/ with the
 * reference's own header names.  Prints the plane and one line per object for the test to compare with the Python path.
 *
 *   kinect_grasp_like <cfg> <weights> <frame.u8: h w c int32 header + bytes>
 *                     <depth.bin: dh dw int32 header + uint16 depth + uint8 body + float map[H][W][2] + float table[dh][dw][2]>
 *                     <thresh> <far_m> <dist_m> <iters> <seed>
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
    if (argc < 10) { fprintf(stderr, "usage: kinect_grasp_like cfg weights frame.u8 depth.bin thresh far_m dist_m iters seed\n"); return 2; }
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
    y2_plane_opts opts = { (float)atof(argv[6]), (float)atof(argv[7]), atoi(argv[8]), (unsigned)strtoul(argv[9], NULL, 10), NULL };

    network net = parse_network_cfg(argv[1]);
    load_weights(&net, argv[2]);
    set_batch_network(&net, 1);
    layer l = net.layers[net.n - 1];
    const int total = l.w * l.h * l.n;
    int i, j;
    char **names = calloc(l.classes, sizeof(char *));
    for (i = 0; i < l.classes; ++i) { names[i] = malloc(32); snprintf(names[i], 32, "class%d", i); }

    if (y2_depth_set_camera_table(net, table, dh, dw) != 0) return 3;    /* once */
    if (y2_depth_set_plane_removal(net, &opts) != 0) return 3;           /* once: desk_seg(1.0) on every frame from here */
    if (y2_depth_set_event(net, Y2_EVENT_GRASP) != 0) return 3;

    y2_depth_frame df = { depth, body, map, dh, dw, H, W };               /* every frame */
    if (y2_depth_upload(net, &df) != 0) return 3;

    y2_region item;
    item.data = frame; item.h = H; item.w = W; item.c = CH; item.step = W * CH;
    item.x = item.y = item.rw = item.rh = 0;
    object *objs = calloc(total, sizeof(object));
    int count = 0;
    test_detector_regions_depth(names, net, &item, 1, NULL, thresh, &objs, &count);

    y2_plane pl;
    if (y2_depth_plane(net, &pl) != 0) return 3;
    printf("PLANE %d %d %d %d %d %.17g %.17g %.17g %.17g\n", pl.found, pl.best, pl.valid_points, pl.best_count, pl.removed, pl.a, pl.b,
           pl.c, pl.d);
    printf("COUNT %d\n", count);
    for (j = 0; j < count; ++j) {
        const object *o = &objs[j];
        printf("OBJ %d %s %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %d %d\n", o->objClass, o->name, o->prob, o->x, o->y, o->w,
               o->h, o->CameraX, o->CameraY, o->CameraZ, o->CameraWidth, o->CameraHeight, (int)o->flagBelong2Person, o->bodyId);
    }
    free_network(net);
    return 0;
}
