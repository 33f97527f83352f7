/* A drop-in user of the reference's rnn.c entry points, compiled against include/ with the reference's own header
 * names: it generates text with test_char_rnn (with a token file), or scores / vectorises stdin.
 *
 *   char_rnn_gen test  <cfg> <weights> <num> <seed> <temperature> <rseed> [token file]
 *   char_rnn_gen valid <cfg> <weights> <seed>   < text
 *   char_rnn_gen vec   <cfg> <weights> <seed>   < lines
 *   char_rnn_gen tokens <token file>            (prints what read_tokens read) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "network.h"
#include "parser.h"
#include "cuda.h"
#include "utils.h"

int main(int argc, char **argv)
{
    if (argc >= 3 && !strcmp(argv[1], "tokens")) {
        size_t n = 0, i;
        char **t = read_tokens(argv[2], &n);
        if (!t) return 3;
        for (i = 0; i < n; ++i) printf("%zu:%s\n", i, t[i]);
        return 0;
    }
    if (argc < 5) { fprintf(stderr, "usage: char_rnn_gen test|valid|vec cfg weights ...\n"); return 2; }
    cuda_set_device(0);
    if (!strcmp(argv[1], "test") && argc >= 8)
        test_char_rnn(argv[2], argv[3], atoi(argv[4]), argv[5], (float)atof(argv[6]), atoi(argv[7]), argc > 8 ? argv[8] : 0);
    else if (!strcmp(argv[1], "valid")) valid_char_rnn(argv[2], argv[3], argv[4]);
    else if (!strcmp(argv[1], "vec")) vec_char_rnn(argv[2], argv[3], argv[4]);
    else return 2;
    return 0;
}
