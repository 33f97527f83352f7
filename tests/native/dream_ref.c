/*
 * dream_ref.c -- TEST INFRASTRUCTURE ONLY (never linked by the product).
 *
 * A small driver, written for this repository, around the network half of the reference's optimize_picture
 * (nightmare.c:48-78, CPU branch): resize_network, forward_network, the copy of the last output into its delta, the
 * reference's own calculate_loss (nightmare.c is compiled next to this file from where it lies; the image.c symbols its
 * other functions name stay unresolved and are never called) and backward_network with a zeroed state.delta.
 * tests/golden/gen_dream_golden.py compiles it against the reference library the oracle recipe builds and stores what it
 * writes.  Raw little-endian float32 files.
 *
 *   dream_ref step <cfg> <weights> <max_layer> <w> <h> <thresh> <input.bin> <outdir>
 *       input.bin is the already built network input [c][h][w].  Writes per layer i <= max_layer l<i>_output.bin and
 *       l<i>_delta.bin ([c][h][w], the delta as backward_network leaves it) and grad.bin, the image gradient [c][h][w].
 *   dream_ref time <cfg> <weights> <max_layer> <w> <h> <thresh> <nsteps>
 *       the same on one fixed pattern in [0, 1); prints the wall-clock seconds of each pass (tools/nightmare_latency.py).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "network.h"
#include "parser.h"
#include "blas.h"

int gpu_index = -1;      /* cuda.h: defined by the reference's CLI */

void calculate_loss(float *output, float *delta, int n, float thresh);      /* nightmare.c:23 */

static void put(const char *dir, const char *name, const float *p, size_t n)
{
    char path[1024];
    FILE *f;
    snprintf(path, sizeof path, "%s/%s", dir, name);
    f = fopen(path, "wb");
    if (!f) { fprintf(stderr, "dream_ref: cannot write %s\n", path); exit(2); }
    fwrite(p, sizeof(float), n, f);
    fclose(f);
}

static network open_net(char **argv, int *max_layer)
{
    network net = parse_network_cfg(argv[2]);
    load_weights(&net, argv[3]);
    set_batch_network(&net, 1);
    *max_layer = atoi(argv[4]);
    if (*max_layer < 0 || *max_layer >= net.n) { fprintf(stderr, "dream_ref: max_layer %d of %d\n", *max_layer, net.n); exit(2); }
    net.n = *max_layer + 1;                                 /* nightmare.c:38 */
    resize_network(&net, atoi(argv[5]), atoi(argv[6]));     /* nightmare.c:48 */
    return net;
}

static void pass(network net, float *input, float *delta, float thresh)
{
    network_state state = {0};
    layer last = net.layers[net.n - 1];
    memset(delta, 0, (size_t)net.w * net.h * net.c * sizeof(float));
    state.input = input;
    state.delta = delta;
    forward_network(net, state);
    copy_cpu(last.outputs, last.output, 1, last.delta, 1);
    calculate_loss(last.output, last.delta, last.outputs, thresh);
    backward_network(net, state);
}

int main(int argc, char **argv)
{
    int max_layer, i, k;
    if (argc == 10 && !strcmp(argv[1], "step")) {
        network net = open_net(argv, &max_layer);
        const size_t n = (size_t)net.w * net.h * net.c;
        float *x = malloc(n * sizeof(float)), *g = malloc(n * sizeof(float));
        FILE *f = fopen(argv[8], "rb");
        if (!f || fread(x, sizeof(float), n, f) != n) { fprintf(stderr, "dream_ref: cannot read %zu floats from %s\n", n, argv[8]); return 2; }
        fclose(f);
        pass(net, x, g, atof(argv[7]));
        for (i = 0; i <= max_layer; ++i) {
            char name[64];
            layer l = net.layers[i];
            snprintf(name, sizeof name, "l%d_output.bin", i);
            put(argv[9], name, l.output, l.outputs);
            snprintf(name, sizeof name, "l%d_delta.bin", i);
            put(argv[9], name, l.delta, l.outputs);
        }
        put(argv[9], "grad.bin", g, n);
        return 0;
    }
    if (argc == 9 && !strcmp(argv[1], "time")) {
        network net = open_net(argv, &max_layer);
        const size_t n = (size_t)net.w * net.h * net.c;
        float *x = malloc(n * sizeof(float)), *g = malloc(n * sizeof(float));
        for (i = 0; (size_t)i < n; ++i) x[i] = (float)(((unsigned)i * 2654435761u) % 1000u) / 1000.f;
        for (k = 0; k < atoi(argv[8]); ++k) {
            struct timespec t0, t1;
            clock_gettime(CLOCK_MONOTONIC, &t0);
            pass(net, x, g, atof(argv[7]));
            clock_gettime(CLOCK_MONOTONIC, &t1);
            printf("pass %d seconds %.4f\n", k + 1, (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec));
            fflush(stdout);
        }
        return 0;
    }
    fprintf(stderr, "usage: dream_ref step <cfg> <weights> <max_layer> <w> <h> <thresh> <input.bin> <outdir> | "
                    "time <cfg> <weights> <max_layer> <w> <h> <thresh> <nsteps>\n");
    return 2;
}
