/*
 * train_v1_ref.c -- TEST INFRASTRUCTURE ONLY (never linked by the product).
 *
 * The YOLOv1 counterpart of train_det_ref.c: a small driver, written for this repository, around the reference's own
 * compiled training path (parse_network_cfg, load_weights, train_network_datum through the reference's headers) for
 * networks that end in [detection].  tests/golden/gen_train_v1_golden.py compiles it against the reference library the
 * oracle recipe builds and stores what it writes.  Raw little-endian float32 files.
 *
 *   train_v1_ref steps <cfg> <weights> <indir> <nsteps> <outdir>
 *       Step k = 1..nsteps reads <indir>/x_k.bin ([batch][c][h][w]) and <indir>/y_k.bin ([batch][l.truths] of the last
 *       layer: per cell is-object, the class row, x, y, w, h), calls srand(k) -- the [dropout] layers draw rand() -- and
 *       train_network_datum, and writes <outdir>/s<k>_loss.bin and, per layer i, s<k>_l<i>_output.bin and _delta.bin plus,
 *       for a convolution or a dense layer, x, x_norm, mean, variance, mean_delta, variance_delta, weight_updates,
 *       bias_updates, scale_updates, weights, biases, scales, rolling_mean, rolling_variance; for a [dropout] only its
 *       rand (its output and delta are the layer's in front).  After the last step it predicts x_1 in inference mode
 *       (network_predict) -> <outdir>/predict.bin.  What the detection layer prints goes to stdout untouched.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "network.h"
#include "parser.h"

int gpu_index = -1;      /* cuda.h: defined by the reference's CLI */

static void put(const char *dir, const char *name, const void *p, size_t bytes)
{
    char path[1024];
    FILE *f;
    if (!p) return;
    snprintf(path, sizeof path, "%s/%s", dir, name);
    f = fopen(path, "wb");
    if (!f) { fprintf(stderr, "train_v1_ref: cannot write %s\n", path); exit(2); }
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
    if (!f || fread(x, sizeof(float), n, f) != n) { fprintf(stderr, "train_v1_ref: cannot read %zu floats from %s\n", n, path); exit(2); }
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
    for (k = 1; k <= nsteps; ++k) {
        float *x = get_floats(argv[4], "x", k, (size_t)net.batch * net.inputs);
        float *y = get_floats(argv[4], "y", k, (size_t)net.batch * net.layers[net.n - 1].truths);
        char name[64];
        float loss;
        srand(k);
        loss = train_network_datum(net, x, y);
        snprintf(name, sizeof name, "s%d_loss.bin", k);
        put(out, name, &loss, sizeof loss);
        for (i = 0; i < net.n; ++i) {
            layer l = net.layers[i];
            const size_t outs = (size_t)l.batch * l.outputs;
            size_t nw;
            if (l.type == DROPOUT) { dump(out, k, i, "rand", l.rand, outs); continue; }
            dump(out, k, i, "output", l.output, outs);
            dump(out, k, i, "delta", l.delta, outs);
            if (l.type != CONVOLUTIONAL && l.type != CONNECTED) continue;
            nw = l.type == CONNECTED ? (size_t)l.outputs * l.inputs : (size_t)l.n * l.c * l.size * l.size;
            if (l.type == CONNECTED) l.n = l.outputs;
            if (l.batch_normalize) {
                dump(out, k, i, "x", l.x, outs);
                dump(out, k, i, "x_norm", l.x_norm, outs);
                dump(out, k, i, "mean", l.mean, l.n);
                dump(out, k, i, "variance", l.variance, l.n);
                dump(out, k, i, "mean_delta", l.mean_delta, l.n);
                dump(out, k, i, "variance_delta", l.variance_delta, l.n);
                dump(out, k, i, "scale_updates", l.scale_updates, l.n);
                dump(out, k, i, "scales", l.scales, l.n);
                dump(out, k, i, "rolling_mean", l.rolling_mean, l.n);
                dump(out, k, i, "rolling_variance", l.rolling_variance, l.n);
            }
            dump(out, k, i, "weight_updates", l.weight_updates, nw);
            dump(out, k, i, "bias_updates", l.bias_updates, l.n);
            dump(out, k, i, "weights", l.weights, nw);
            dump(out, k, i, "biases", l.biases, l.n);
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

int main(int argc, char **argv)
{
    if (argc == 7 && !strcmp(argv[1], "steps")) return cmd_steps(argv);
    fprintf(stderr, "usage: train_v1_ref steps <cfg> <weights> <indir> <nsteps> <outdir>\n");
    return 2;
}
