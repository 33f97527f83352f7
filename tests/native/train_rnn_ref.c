/*
 * train_rnn_ref.c -- TEST INFRASTRUCTURE ONLY (never linked by the product).
 *
 * The char-rnn counterpart of train_v1_ref.c: a small driver, written for this repository, around the reference's own
 * compiled training path (parse_network_cfg, load_weights, train_network_datum through the reference's headers) for
 * networks of [rnn] layers followed by [connected], [softmax] and [cost].  tests/golden/gen_train_rnn_golden.py compiles it
 * against the reference library the oracle recipe builds and stores what it writes.  Raw little-endian float32 files.
 *
 *   train_rnn_ref steps <cfg> <weights> <indir> <nsteps> <outdir>
 *       Step k = 1..nsteps reads <indir>/x_k.bin ([net.batch][inputs], rows step-major) and <indir>/y_k.bin
 *       ([net.batch][outputs]), calls train_network_datum and writes <outdir>/s<k>_loss.bin and, per layer i,
 *       s<k>_l<i>_output.bin and _delta.bin; for a [connected] layer its x, x_norm, mean, variance, mean_delta,
 *       variance_delta, weight_updates, bias_updates, scale_updates, weights, biases, scales, rolling_mean, rolling_variance;
 *       for an [rnn] layer s<k>_l<i>_state.bin (the T+1 slots) and the same arrays of its three sub-layers as
 *       s<k>_l<i>_input.<array>.bin, _self.<array>.bin, _output.<array>.bin, over all T*B rows.  After the last step it
 *       predicts x_1 in inference mode (network_predict) -> <outdir>/predict.bin.
 *   train_rnn_ref losses <cfg> <weights> <indir> <nsteps> <outdir>
 *       The same steps, writing only <outdir>/losses.bin (nsteps floats) and the wall time of the steps in seconds to stdout.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

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
    if (!f) { fprintf(stderr, "train_rnn_ref: cannot write %s\n", path); exit(2); }
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
    if (!f || fread(x, sizeof(float), n, f) != n) { fprintf(stderr, "train_rnn_ref: cannot read %zu floats from %s\n", n, path); exit(2); }
    fclose(f);
    return x;
}

static void dump(const char *dir, int k, int i, const char *sub, const char *what, const float *p, size_t n)
{
    char name[160];
    snprintf(name, sizeof name, "s%d_l%d_%s%s.bin", k, i, sub, what);
    put(dir, name, p, n * sizeof(float));
}

/* a [connected] layer over `rows` rows; sub is "" or "input." / "self." / "output." */
static void dump_connected(const char *dir, int k, int i, const char *sub, layer l, size_t rows)
{
    const size_t outs = rows * l.outputs, nw = (size_t)l.outputs * l.inputs, n = l.outputs;
    dump(dir, k, i, sub, "output", l.output, outs);
    dump(dir, k, i, sub, "delta", l.delta, outs);
    if (l.batch_normalize) {
        dump(dir, k, i, sub, "x", l.x, outs);
        dump(dir, k, i, sub, "x_norm", l.x_norm, outs);
        dump(dir, k, i, sub, "mean", l.mean, n);
        dump(dir, k, i, sub, "variance", l.variance, n);
        dump(dir, k, i, sub, "mean_delta", l.mean_delta, n);
        dump(dir, k, i, sub, "variance_delta", l.variance_delta, n);
        dump(dir, k, i, sub, "scale_updates", l.scale_updates, n);
        dump(dir, k, i, sub, "scales", l.scales, n);
        dump(dir, k, i, sub, "rolling_mean", l.rolling_mean, n);
        dump(dir, k, i, sub, "rolling_variance", l.rolling_variance, n);
    }
    dump(dir, k, i, sub, "weight_updates", l.weight_updates, nw);
    dump(dir, k, i, sub, "bias_updates", l.bias_updates, n);
    dump(dir, k, i, sub, "weights", l.weights, nw);
    dump(dir, k, i, sub, "biases", l.biases, n);
}

static int cmd_steps(char **argv, int all)
{
    network net = parse_network_cfg(argv[2]);
    const int nsteps = atoi(argv[5]);
    const char *out = argv[6];
    float *x1 = NULL, *losses = calloc(nsteps, sizeof(float));
    double spent = 0;
    int k, i;
    load_weights(&net, argv[3]);
    for (k = 1; k <= nsteps; ++k) {
        float *x = get_floats(argv[4], "x", k, (size_t)net.batch * net.inputs);
        float *y = get_floats(argv[4], "y", k, (size_t)net.batch * net.outputs);
        struct timespec t0, t1;
        char name[64];
        float loss;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        loss = train_network_datum(net, x, y);
        clock_gettime(CLOCK_MONOTONIC, &t1);
        spent += (t1.tv_sec - t0.tv_sec) + (t1.tv_nsec - t0.tv_nsec) * 1e-9;
        losses[k - 1] = loss;
        if (all) {
            snprintf(name, sizeof name, "s%d_loss.bin", k);
            put(out, name, &loss, sizeof loss);
        }
        for (i = 0; all && i < net.n; ++i) {
            layer l = net.layers[i];
            if (l.type == RNN) {
                const size_t rows = (size_t)l.batch * l.steps;
                dump(out, k, i, "", "state", l.state, (size_t)l.batch * l.hidden * (l.steps + 1));
                dump(out, k, i, "", "output", l.output, rows * l.outputs);
                dump(out, k, i, "", "delta", l.delta, rows * l.outputs);
                dump_connected(out, k, i, "input.", *l.input_layer, rows);
                dump_connected(out, k, i, "self.", *l.self_layer, rows);
                dump_connected(out, k, i, "output.", *l.output_layer, rows);
            } else if (l.type == CONNECTED) {
                dump_connected(out, k, i, "", l, l.batch);
            } else {
                dump(out, k, i, "", "output", l.output, (size_t)l.batch * l.outputs);
                dump(out, k, i, "", "delta", l.delta, (size_t)l.batch * l.outputs);
            }
        }
        if (k == 1) x1 = x; else free(x);
        free(y);
    }
    if (!all) {
        put(out, "losses.bin", losses, nsteps * sizeof(float));
        printf("%.6f\n", spent);
    } else if (x1) {
        float *p = network_predict(net, x1);
        put(out, "predict.bin", p, (size_t)net.batch * get_network_output_size(net) * sizeof(float));
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 7 && !strcmp(argv[1], "steps")) return cmd_steps(argv, 1);
    if (argc == 7 && !strcmp(argv[1], "losses")) return cmd_steps(argv, 0);
    fprintf(stderr, "usage: train_rnn_ref steps|losses <cfg> <weights> <indir> <nsteps> <outdir>\n");
    return 2;
}
