/* A character-RNN caller written like test_char_rnn (rnn.c:225-280), compiled against include/ with the reference's
 * own header names: parse_network_cfg, load_weights, the temperature written on every layer, then network_predict
 * once per character -- here teacher-forced from a file of input rows instead of sampled.  After the last step it calls
 * reset_rnn_state for every item and predicts the first step again.
 *
 *   char_rnn_like <cfg> <weights> <rows.f32: steps x batch x inputs> <steps> <temperature> <out.f32>
 *
 * out.f32 holds steps + 1 blocks of batch x outputs floats: one per call, the last one after the reset. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "network.h"
#include "parser.h"
#include "cuda.h"
#include "utils.h"

int main(int argc, char **argv)
{
    int i, t;
    if (argc < 7) { fprintf(stderr, "usage: char_rnn_like cfg weights rows.f32 steps temperature out.f32\n"); return 2; }
    cuda_set_device(0);
    network net = parse_network_cfg(argv[1]);
    load_weights(&net, argv[2]);
    const int steps = atoi(argv[4]);
    const float temp = (float)atof(argv[5]);
    for (i = 0; i < net.n; ++i) net.layers[i].temperature = temp;     /* rnn.c:244 */
    const int inputs = get_network_input_size(net), outputs = get_network_output_size(net);
    const size_t in_floats = (size_t)net.batch * inputs, out_floats = (size_t)net.batch * outputs;
    float *rows = malloc((size_t)steps * in_floats * sizeof(float));
    FILE *f = fopen(argv[3], "rb");
    if (!f || fread(rows, sizeof(float), (size_t)steps * in_floats, f) != (size_t)steps * in_floats) { fprintf(stderr, "bad rows file\n"); return 2; }
    fclose(f);
    float *input = calloc(in_floats, sizeof(float));
    FILE *out = fopen(argv[6], "wb");
    if (!out) { fprintf(stderr, "cannot write %s\n", argv[6]); return 2; }
    for (t = 0; t <= steps; ++t) {
        if (t == steps) reset_rnn_state(net, -1);                     /* every sequence starts again */
        memcpy(input, rows + (size_t)(t == steps ? 0 : t) * in_floats, in_floats * sizeof(float));
        float *p = network_predict(net, input);
        if (!p) { fprintf(stderr, "network_predict failed\n"); return 3; }
        fwrite(p, sizeof(float), out_floats, out);
    }
    fclose(out);
    printf("inputs %d outputs %d batch %d steps %d\n", inputs, outputs, net.batch, steps);
    free(rows); free(input);
    free_network(net);
    return 0;
}
