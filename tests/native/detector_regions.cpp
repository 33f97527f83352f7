// Detector::detect_regions from a yolo_console_dll.cpp-style caller: the whole frame and two hand crops in one call,
// compared with detect_frame on the host-copied crops, and the batch-1 network checked untouched afterwards.
//   detector_regions <cfg> <weights> <frame.u8: h w c int32 header + bytes> <thresh> rx1 ry1 rw1 rh1 rx2 ry2 rw2 rh2
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "yolo_v2_class.hpp"

static bool same(const std::vector<bbox_t> &a, const std::vector<bbox_t> &b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].x != b[i].x || a[i].y != b[i].y || a[i].w != b[i].w || a[i].h != b[i].h || a[i].prob != b[i].prob ||
            a[i].obj_id != b[i].obj_id)
            return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 13) return 2;
    FILE *f = std::fopen(argv[3], "rb");
    int hdr[3];
    if (!f || std::fread(hdr, sizeof(int), 3, f) != 3) return 2;
    const int H = hdr[0], W = hdr[1], C = hdr[2];
    std::vector<unsigned char> frame((size_t)H * W * C);
    if (std::fread(frame.data(), 1, frame.size(), f) != frame.size()) return 2;
    std::fclose(f);
    const float thresh = (float)std::atof(argv[4]);

    Detector det(argv[1], argv[2], 0);
    std::vector<frame_region_t> items(3);
    for (int i = 0; i < 3; ++i) items[i] = frame_region_t{frame.data(), W, H, C, W * C, 0, 0, 0, 0};
    for (int i = 1; i < 3; ++i) {
        items[i].x = std::atoi(argv[1 + 4 * i]); items[i].y = std::atoi(argv[2 + 4 * i]);
        items[i].rw = std::atoi(argv[3 + 4 * i]); items[i].rh = std::atoi(argv[4 + 4 * i]);
    }

    const std::vector<bbox_t> before = det.detect_frame(frame.data(), W, H, C, W * C, thresh, true);
    // two items first, then three: the regions network grows once; the crops' results do not depend on it
    std::vector<frame_region_t> two(items.begin() + 1, items.end());
    const std::vector<std::vector<bbox_t>> r2 = det.detect_regions(two, thresh, true);
    const std::vector<std::vector<bbox_t>> r3 = det.detect_regions(items, thresh, true);
    std::printf("GREW %d\n", (r2.size() == 2 && same(r2[0], r3[1]) && same(r2[1], r3[2])) ? 1 : 0);
    for (int i = 0; i < 3; ++i)
        for (const bbox_t &b : r3[i]) std::printf("REG %d %u %u %u %u %.9g %u\n", i, b.x, b.y, b.w, b.h, b.prob, b.obj_id);

    for (int i = 0; i < 3; ++i) {
        const frame_region_t &it = items[i];
        const int rx = it.rw ? it.x : 0, ry = it.rw ? it.y : 0, rw = it.rw ? it.rw : W, rh = it.rw ? it.rh : H;
        std::vector<unsigned char> crop((size_t)rw * rh * C);
        for (int y = 0; y < rh; ++y)
            for (int x = 0; x < rw * C; ++x) crop[(size_t)y * rw * C + x] = frame[((size_t)(ry + y) * W + rx) * C + x];
        for (const bbox_t &b : det.detect_frame(crop.data(), rw, rh, C, rw * C, thresh, true))
            std::printf("CROP %d %u %u %u %u %.9g %u %d %d\n", i, b.x + rx, b.y + ry, b.w, b.h, b.prob, b.obj_id, rx, ry);
    }
    const std::vector<bbox_t> after = det.detect_frame(frame.data(), W, H, C, W * C, thresh, true);
    std::printf("UNCHANGED %d\n", (same(before, after) && same(before, r3[0])) ? 1 : 0);
    return 0;
}
