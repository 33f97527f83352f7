/*
 * hier_ref.c -- TEST INFRASTRUCTURE ONLY (never linked by the product).
 *
 * A small driver, written for this repository, that calls the reference's own compiled tree functions through the
 * reference's headers (tree.h: read_tree, change_leaves, get_hierarchy_probability, hierarchy_predictions; utils.h:
 * top_k).  tests/golden/gen_hier_golden.py compiles it against the reference library the oracle recipe builds and stores
 * what it writes.  Raw little-endian int32 / float32 files.
 *
 *   hier_ref tree <tree file> <outdir>
 *       meta.txt (n, groups), group_size.bin, group_offset.bin, group.bin, leaf.bin, parent.bin as read_tree made them
 *   hier_ref rows <tree file> <rows.bin> <leaf list> <outdir>
 *       rows.bin holds k rows of n conditional probabilities.  Per row: hp0.bin / hp1.bin = hierarchy_predictions with
 *       only_leaves 0 / 1, ghp.bin = get_hierarchy_probability of every node, top3.bin = top_k(hp0 row, n, 3); then
 *       change_leaves(tree, leaf list): leaf2.bin = the new flags, hp1b.bin = hierarchy_predictions(.., 1) with them
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tree.h"
#include "utils.h"

int gpu_index = -1;      /* cuda.h: defined by the reference's CLI */

static void put(const char *dir, const char *name, const void *p, size_t bytes)
{
    char path[1024];
    FILE *f;
    snprintf(path, sizeof path, "%s/%s", dir, name);
    f = fopen(path, "wb");
    if (!f) { fprintf(stderr, "hier_ref: cannot write %s\n", path); exit(2); }
    fwrite(p, 1, bytes, f);
    fclose(f);
}

static float *get_floats(const char *path, size_t *n)
{
    FILE *f = fopen(path, "rb");
    long bytes;
    float *x;
    if (!f) { fprintf(stderr, "hier_ref: cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END);
    bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    x = malloc(bytes > 0 ? bytes : 4);
    if (fread(x, 1, bytes, f) != (size_t)bytes) { fprintf(stderr, "hier_ref: short read %s\n", path); exit(2); }
    fclose(f);
    *n = bytes / sizeof(float);
    return x;
}

static int cmd_tree(char **argv)
{
    tree *t = read_tree(argv[2]);
    char meta[64];
    snprintf(meta, sizeof meta, "n %d\ngroups %d\n", t->n, t->groups);
    put(argv[3], "meta.txt", meta, strlen(meta));
    put(argv[3], "group_size.bin", t->group_size, t->groups * sizeof(int));
    put(argv[3], "group_offset.bin", t->group_offset, t->groups * sizeof(int));
    put(argv[3], "group.bin", t->group, t->n * sizeof(int));
    put(argv[3], "leaf.bin", t->leaf, t->n * sizeof(int));
    put(argv[3], "parent.bin", t->parent, t->n * sizeof(int));
    return 0;
}

static int cmd_rows(char **argv)
{
    tree *t = read_tree(argv[2]);
    size_t total = 0, k, r;
    float *rows = get_floats(argv[3], &total);
    const int n = t->n;
    float *hp0, *hp1, *hp1b, *ghp;
    int *top3, c;
    if (n <= 0 || total % n) { fprintf(stderr, "hier_ref: %zu floats are no rows of %d\n", total, n); return 2; }
    k = total / n;
    hp0 = malloc(total * sizeof(float)); hp1 = malloc(total * sizeof(float)); hp1b = malloc(total * sizeof(float));
    ghp = malloc(total * sizeof(float)); top3 = malloc(k * 3 * sizeof(int));
    memcpy(hp0, rows, total * sizeof(float)); memcpy(hp1, rows, total * sizeof(float)); memcpy(hp1b, rows, total * sizeof(float));
    for (r = 0; r < k; ++r) {
        hierarchy_predictions(hp0 + r * n, n, t, 0);
        hierarchy_predictions(hp1 + r * n, n, t, 1);
        for (c = 0; c < n; ++c) ghp[r * n + c] = get_hierarchy_probability(rows + r * n, t, c);
        top_k(hp0 + r * n, n, 3, top3 + r * 3);
    }
    change_leaves(t, argv[4]);
    for (r = 0; r < k; ++r) hierarchy_predictions(hp1b + r * n, n, t, 1);
    put(argv[5], "hp0.bin", hp0, total * sizeof(float));
    put(argv[5], "hp1.bin", hp1, total * sizeof(float));
    put(argv[5], "hp1b.bin", hp1b, total * sizeof(float));
    put(argv[5], "ghp.bin", ghp, total * sizeof(float));
    put(argv[5], "top3.bin", top3, k * 3 * sizeof(int));
    put(argv[5], "leaf2.bin", t->leaf, n * sizeof(int));
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "tree")) return cmd_tree(argv);
    if (argc == 6 && !strcmp(argv[1], "rows")) return cmd_rows(argv);
    fprintf(stderr, "usage: hier_ref tree <tree> <outdir> | rows <tree> <rows.bin> <leaf list> <outdir>\n");
    return 2;
}
