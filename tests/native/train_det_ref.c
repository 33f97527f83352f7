/*
 * train_det_ref.c -- TEST INFRASTRUCTURE ONLY (never linked by the product).
 *
 * The detector's counterpart of train_ref.c: a small driver, written for this repository, around the reference's own
 * compiled training path (parse_network_cfg, load_weights, train_network_datum through the reference's headers) for
 * networks that end in [region].  tests/golden/gen_train_det_golden.py compiles it against the reference library the
 * oracle recipe builds and stores what it writes.  Raw little-endian float32 files.
 *
 *   train_det_ref steps <cfg> <weights> <indir> <nsteps> <outdir> <seen>
 *       *net.seen starts at <seen>.  Step k = 1..nsteps reads <indir>/x_k.bin ([batch][c][h][w]) and <indir>/y_k.bin
 *       ([batch][l.truths] of the last layer: rows of x, y, w, h, class), calls train_network_datum and writes
 *       <outdir>/s<k>_loss.bin and, per layer i, <outdir>/s<k>_l<i>_output.bin and _delta.bin plus, for a convolution,
 *       x, x_norm, mean, variance, mean_delta, variance_delta, weight_updates, bias_updates, scale_updates, weights,
 *       biases, scales, rolling_mean, rolling_variance.  After the last step it predicts x_1 in inference mode
 *       (network_predict) -> <outdir>/predict.bin.  What the region layer prints goes to stdout untouched.
 *   train_det_ref time <cfg> <weights> <nsteps>
 *       nsteps train_network_datum calls on one fixed batch (a fixed pattern in [-1, 1); three truths per image); prints
 *       the wall-clock seconds of each call and its loss (tools/train_latency.py).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "network.h"
#include "parser.h"

int gpu_index = -1;      /* cuda.h: defined by the reference's CLI */

static size_t truth_floats(network net)
{
    const layer last = net.layers[net.n - 1];
    return (size_t)net.batch * (last.truths ? last.truths : last.inputs);
}

static void put(const char *dir, const char *name, const void *p, size_t bytes)
{
    char path[1024];
    FILE *f;
    if (!p) return;
    snprintf(path, sizeof path, "%s/%s", dir, name);
    f = fopen(path, "wb");
    if (!f) { fprintf(stderr, "train_det_ref: cannot write %s\n", path); exit(2); }
    fwrite(p, 1, bytes, f);
    fclose(f);
}

static float *get_floats(const char *dir, const char *stem, int k, size_t n)
{
    char path[1024];
    FILE *f;
    float *x = malloc(n * sizeof(float));
    snprintf(path, sizeof path, "%s/%s_%d.bin", dir, stem, k);
    f = fopen(path, "rb");
    if (!f || fread(x, sizeof(float), n, f) != n) { fprintf(stderr, "train_det_ref: cannot read %zu floats from %s\n", n, path); exit(2); }
    fclose(f);
    return x;
}

static void dump(const char *dir, int k, int i, const char *what, const float *p, size_t n)
{
    char name[128];
    snprintf(name, sizeof name, "s%d_l%d_%s.bin", k, i, what);
    put(dir, name, p, n * sizeof(float));
}

static int cmd_steps(char **argv)
{
    network net = parse_network_cfg(argv[2]);
    const int nsteps = atoi(argv[5]);
    const char *out = argv[6];
    float *x1 = NULL;
    int k, i;
    load_weights(&net, argv[3]);
    *net.seen = atoi(argv[7]);
    for (k = 1; k <= nsteps; ++k) {
        float *x = get_floats(argv[4], "x", k, (size_t)net.batch * net.inputs);
        float *y = get_floats(argv[4], "y", k, truth_floats(net));
        float loss = train_network_datum(net, x, y);
        char name[64];
        snprintf(name, sizeof name, "s%d_loss.bin", k);
        put(out, name, &loss, sizeof loss);
        for (i = 0; i < net.n; ++i) {
            layer l = net.layers[i];
            const size_t outs = (size_t)l.batch * l.outputs;
            dump(out, k, i, "output", l.output, outs);
            dump(out, k, i, "delta", l.delta, outs);
            if (l.type != CONVOLUTIONAL) continue;
            dump(out, k, i, "x", l.x, outs);
            dump(out, k, i, "x_norm", l.x_norm, outs);
            dump(out, k, i, "mean", l.mean, l.n);
            dump(out, k, i, "variance", l.variance, l.n);
            dump(out, k, i, "mean_delta", l.mean_delta, l.n);
            dump(out, k, i, "variance_delta", l.variance_delta, l.n);
            dump(out, k, i, "weight_updates", l.weight_updates, (size_t)l.n * l.c * l.size * l.size);
            dump(out, k, i, "bias_updates", l.bias_updates, l.n);
            dump(out, k, i, "scale_updates", l.scale_updates, l.n);
            dump(out, k, i, "weights", l.weights, (size_t)l.n * l.c * l.size * l.size);
            dump(out, k, i, "biases", l.biases, l.n);
            dump(out, k, i, "scales", l.scales, l.n);
            dump(out, k, i, "rolling_mean", l.rolling_mean, l.n);
            dump(out, k, i, "rolling_variance", l.rolling_variance, l.n);
        }
        if (k == 1) x1 = x; else free(x);
        free(y);
    }
    if (x1) {
        float *p = network_predict(net, x1);
        put(out, "predict.bin", p, (size_t)net.batch * get_network_output_size(net) * sizeof(float));
    }
    return 0;
}

static int cmd_time(char **argv)
{
    network net = parse_network_cfg(argv[2]);
    const layer last = net.layers[net.n - 1];
    const size_t nx = (size_t)net.batch * net.inputs, ny = truth_floats(net);
    float *x = calloc(nx, sizeof(float)), *y = calloc(ny, sizeof(float));
    size_t i;
    int k, t;
    load_weights(&net, argv[3]);
    for (i = 0; i < nx; ++i) x[i] = (float)((i * 2654435761u) % 2001u) / 1000.f - 1.f;
    for (i = 0; i < (size_t)net.batch; ++i)
        for (t = 0; t < 3; ++t) {
            float *r = y + i * last.truths + t * 5;
            r[0] = .2f + .3f * t; r[1] = .7f - .2f * t; r[2] = .1f + .15f * t; r[3] = .4f - .1f * t; r[4] = (float)((i + t) % last.classes);
        }
    for (k = 0; k < atoi(argv[4]); ++k) {
        struct timespec t0, t1;
        float loss;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        loss = train_network_datum(net, x, y);
        clock_gettime(CLOCK_MONOTONIC, &t1);
        printf("step %d seconds %.4f loss %f\n", k + 1, (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec), loss);
        fflush(stdout);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "time")) return cmd_time(argv);
    if (argc == 8 && !strcmp(argv[1], "steps")) return cmd_steps(argv);
    fprintf(stderr, "usage: train_det_ref steps <cfg> <weights> <indir> <nsteps> <outdir> <seen> | time <cfg> <weights> <nsteps>\n");
    return 2;
}
