/* A drop-in user of the reference's training entry points, compiled against include/ with the reference's own header
 * names: the loop of a fine-tuning caller (classifier.c train_classifier without its data loader).
 *
 *   train_like <cfg> <weights> <x.bin> <y.bin> <steps> <out.weights>
 *       x.bin: [batch][c][h][w] floats, y.bin: [batch][outputs]; the same batch every step.  Prints per step
 *       "<batch number>: loss <loss>, rate <rate>"; then predicts x and saves the trained weights. */
#include <stdio.h>
#include <stdlib.h>

#include "network.h"
#include "parser.h"
#include "cuda.h"

static float *read_floats(const char *path, size_t n)
{
    FILE *f = fopen(path, "rb");
    float *x = malloc(n * sizeof(float));
    if (!f || fread(x, sizeof(float), n, f) != n) { fprintf(stderr, "train_like: cannot read %zu floats from %s\n", n, path); exit(2); }
    fclose(f);
    return x;
}

int main(int argc, char **argv)
{
    network net;
    float *x, *y, *p;
    int i, steps;
    if (argc != 7) { fprintf(stderr, "usage: train_like cfg weights x.bin y.bin steps out.weights\n"); return 2; }
    cuda_set_device(0);
    net = parse_network_cfg(argv[1]);
    load_weights(&net, argv[2]);
    x = read_floats(argv[3], (size_t)net.batch * net.inputs);
    y = read_floats(argv[4], (size_t)net.batch * net.layers[net.n - 1].inputs);
    steps = atoi(argv[5]);
    for (i = 0; i < steps; ++i) {
        float loss = train_network_datum(net, x, y);
        printf("%d: loss %f, rate %g, cost %f\n", get_current_batch(net), loss, get_current_rate(net), get_network_cost(net));
    }
    p = network_predict(net, x);
    printf("predict %f\n", p[0]);
    save_weights(net, argv[6]);
    free_network(net);
    return 0;
}
