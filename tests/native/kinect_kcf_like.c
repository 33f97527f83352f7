/* The Kinect loop's tracking between detection frames (KinectUtil_with_cam.cpp:764-803: InitialTracker after a detection
 * frame, test_tracker_img on every frame until the next one) as the application would write it against this library,
 * compiled against include/ with the reference's own header names: one y2_kcf_init_objects, then one
 * y2_kcf_track_objects per frame.  Prints one line per tracked object for a test to compare with the Python path.
 *
 *   kinect_kcf_like <cfg> <frames.u8: n h w c int32 header + n frames> <objects: x y w h per object, relative> ...
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "network.h"
#include "parser.h"
#include "cuda.h"
#include "utils.h"
#include "test_detector.h"

static network net;
static unsigned char *colorMat;
static int imgHeight, imgWidth, imgChannels;

static void InitialTracker(object *RecObjects, int objectNumPerFrame)
{
    y2_kcf_init_objects(net, colorMat, imgHeight, imgWidth, imgChannels, imgWidth * imgChannels, RecObjects, objectNumPerFrame);
}

static void test_tracker_img(object *RecObjects, int *objectNumPerFrame)
{
    y2_kcf_track_objects(net, colorMat, imgHeight, imgWidth, imgChannels, imgWidth * imgChannels, RecObjects, objectNumPerFrame);
}

int main(int argc, char **argv)
{
    int hdr[4], i, k, n_obj, frames;
    object objs[Y2_KCF_MAX_TRACKERS];
    FILE *f;
    size_t bytes;
    if (argc < 7 || (argc - 3) % 4) { fprintf(stderr, "usage: kinect_kcf_like cfg frames.u8 (x y w h) ...\n"); return 2; }
    cuda_set_device(0);
    f = fopen(argv[2], "rb");
    if (!f || fread(hdr, sizeof(int), 4, f) != 4) { fprintf(stderr, "bad frame file\n"); return 2; }
    frames = hdr[0]; imgHeight = hdr[1]; imgWidth = hdr[2]; imgChannels = hdr[3];
    bytes = (size_t)imgHeight * imgWidth * imgChannels;
    colorMat = malloc(bytes);
    n_obj = (argc - 3) / 4;
    if (n_obj > Y2_KCF_MAX_TRACKERS) return 2;
    memset(objs, 0, sizeof objs);
    for (i = 0; i < n_obj; ++i) {
        objs[i].x = (float)atof(argv[3 + 4 * i]); objs[i].y = (float)atof(argv[4 + 4 * i]);
        objs[i].w = (float)atof(argv[5 + 4 * i]); objs[i].h = (float)atof(argv[6 + 4 * i]);
        snprintf(objs[i].name, sizeof objs[i].name, "object%d", i);
        objs[i].prob = 0.5f; objs[i].objClass = i;
    }
    net = parse_network_cfg(argv[1]);
    for (k = 0; k < frames; ++k) {
        if (fread(colorMat, 1, bytes, f) != bytes) { fprintf(stderr, "short frame file\n"); return 2; }
        if (k == 0) { InitialTracker(objs, n_obj); continue; }           /* the detection frame */
        {
            int n = 0;
            test_tracker_img(objs, &n);
            for (i = 0; i < n; ++i)
                printf("TRACK %d %d %s %.9g %.9g %.9g %.9g\n", k, i, objs[i].name, objs[i].x, objs[i].y, objs[i].w, objs[i].h);
        }
    }
    fclose(f);
    y2_kcf_free(net);
    free_network(net);
    free(colorMat);
    return 0;
}
