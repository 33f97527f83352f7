// Detector::upload_depth / set_camera_table / detect_regions_depth from a C++ caller, compiled against include/ like an
// application would: the Kinect loop's frame and two filtered hand crops in one call, every box with its depth fields.
// Prints one line per box for the test to compare with the C API's results.
//
//   detector_depth <cfg> <weights> <frame.u8: h w c int32 header + bytes>
//                  <depth.bin: dh dw int32 header + uint16 depth + uint8 body + float map[H][W][2] + float table[dh][dw][2]>
//                  <thresh> rx1 ry1 rw1 rh1 far1 rx2 ry2 rw2 rh2 far2
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "yolo_v2_class.hpp"

template <class T> static bool read_all(FILE *f, std::vector<T> &v) { return fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv)
{
    if (argc < 16) { fprintf(stderr, "usage: detector_depth cfg weights frame.u8 depth.bin thresh (rx ry rw rh far) x 2\n"); return 2; }
    FILE *f = fopen(argv[3], "rb");
    int hdr[3], dhdr[2];
    if (!f || fread(hdr, sizeof(int), 3, f) != 3) return 2;
    const int H = hdr[0], W = hdr[1], CH = hdr[2];
    std::vector<unsigned char> frame((size_t)H * W * CH);
    if (!read_all(f, frame)) return 2;
    fclose(f);
    f = fopen(argv[4], "rb");
    if (!f || fread(dhdr, sizeof(int), 2, f) != 2) return 2;
    const int dh = dhdr[0], dw = dhdr[1];
    std::vector<unsigned short> depth((size_t)dh * dw);
    std::vector<unsigned char> body((size_t)dh * dw);
    std::vector<float> map((size_t)H * W * 2), table((size_t)dh * dw * 2);
    if (!read_all(f, depth) || !read_all(f, body) || !read_all(f, map) || !read_all(f, table)) return 2;
    fclose(f);

    std::vector<frame_region_t> items(3, frame_region_t{frame.data(), W, H, CH, W * CH, 0, 0, 0, 0});
    std::vector<float> far_m(3, 0.f);
    for (int i = 1; i < 3; ++i) {
        char **a = argv + 6 + 5 * (i - 1);
        items[i].x = atoi(a[0]); items[i].y = atoi(a[1]); items[i].rw = atoi(a[2]); items[i].rh = atoi(a[3]);
        far_m[i] = (float)atof(a[4]);
    }
    try {
        Detector det(argv[1], argv[2], 0);
        det.nms = 0.1f;
        det.set_camera_table(table.data(), dh, dw);
        det.upload_depth(depth_frame_t{depth.data(), body.data(), map.data(), dh, dw, H, W});
        std::vector<std::vector<bbox3d_t>> out = det.detect_regions_depth(items, far_m, (float)atof(argv[5]));
        for (size_t i = 0; i < out.size(); ++i)
            for (const bbox3d_t &b : out[i])
                printf("BOX %zu %u %.9g %u %u %u %u %d %.9g %.9g %.9g %.9g %.9g %.9g %d %d %d\n", i, b.box.obj_id, b.box.prob, b.box.x,
                       b.box.y, b.box.w, b.box.h, (int)b.valid, b.x, b.y, b.z, b.width, b.height, b.avg_mm, b.otsu,
                       (int)b.belongs_to_person, b.body_id);
        // without far_m: the same boxes as detect_regions
        std::vector<std::vector<bbox3d_t>> plain = det.detect_regions_depth(items);
        std::vector<std::vector<bbox_t>> ref = det.detect_regions(items);
        bool same = plain.size() == ref.size();
        for (size_t i = 0; same && i < ref.size(); ++i) {
            same = plain[i].size() == ref[i].size();
            for (size_t j = 0; same && j < ref[i].size(); ++j)
                same = plain[i][j].box.x == ref[i][j].x && plain[i][j].box.y == ref[i][j].y && plain[i][j].box.w == ref[i][j].w &&
                       plain[i][j].box.h == ref[i][j].h && plain[i][j].box.prob == ref[i][j].prob && plain[i][j].box.obj_id == ref[i][j].obj_id;
        }
        printf("UNFILTERED_EQUALS_DETECT_REGIONS %d\n", (int)same);
    } catch (const std::exception &e) {
        fprintf(stderr, "detector_depth: %s\n", e.what());
        return 3;
    }
    return 0;
}
