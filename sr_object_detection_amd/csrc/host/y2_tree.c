/* y2_tree.c -- the classifier side of the WordTree: the reference's tree.c on the host (change_leaves :7,
 * get_hierarchy_probability :27, hierarchy_predictions :37) and hierarchy_predictions on the device copy of the output rows
 * (y2h_hierarchy_rows), for the classifier evaluations and for callers of y2_forward_device. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "y2_internal.h"

/* ------------------------------------------------------------------ */
/* tree.c on the host                                                  */
/* ------------------------------------------------------------------ */
void change_leaves(tree *t, char *leaf_list)     /* tree.c:7-25 */
{
    FILE *fp;
    char **leaves = NULL, *line;
    int n = 0, i, j, found = 0;
    if (!t || !leaf_list) { y2_fail("change_leaves: missing argument"); return; }
    fp = fopen(leaf_list, "r");
    if (!fp) { file_error(leaf_list); return; }
    while ((line = y2_fgetl(fp)) != NULL) {      /* get_paths (data.c:14-26): one entry per line */
        leaves = realloc(leaves, (n + 1) * sizeof(char *));
        leaves[n++] = line;
    }
    fclose(fp);
    for (i = 0; i < t->n; ++i) {
        t->leaf[i] = 0;
        for (j = 0; j < n; ++j)
            if (0 == strcmp(t->name[i], leaves[j])) { t->leaf[i] = 1; ++found; break; }
    }
    fprintf(stderr, "Found %d leaves.\n", found);
    for (j = 0; j < n; ++j) free(leaves[j]);
    free(leaves);
}

/* tree.c:27-35: the absolute probability of node c out of a CONDITIONAL row -- x[c] times x of every ancestor, multiplied
 * from the node upwards (that order is the reference's rounding) */
float get_hierarchy_probability(float *x, tree *hier, int c)
{
    float prob = 1;
    int node;
    for (node = c; node >= 0; node = hier->parent[node]) prob *= x[node];
    return prob;
}

/* tree.c:37-51: a conditional row becomes absolute in place.  Nodes are visited in file order and each is scaled by its
 * parent's CURRENT value: final when the parent stands earlier in the file, still conditional when it stands later.
 * With only_leaves every inner node is then cleared. */
void hierarchy_predictions(float *predictions, int n, tree *hier, int only_leaves)
{
    const int *up = hier->parent;
    int node;
    for (node = 0; node < n; ++node)
        if (up[node] >= 0) predictions[node] = predictions[node] * predictions[up[node]];
    for (node = 0; only_leaves && node < n; ++node)
        if (hier->leaf[node] == 0) predictions[node] = 0;
}

/* ------------------------------------------------------------------ */
/* on the device                                                       */
/* ------------------------------------------------------------------ */
/* The hierarchy the device can apply is the tree its output [softmax] layer was planned with, covering the whole output row:
 * its tables are in HBM and were checked against the row (y2_softmax_tree_check).  Any other net.hierarchy -- a tree hung on
 * a flat classifier, a head with groups > 1, whose rows are outputs/groups long -- is refused: NULL when net.hierarchy is
 * fine, otherwise the sentence (written into buf).  Needs no device. */
const char *y2_hierarchy_refusal(const network *net, char *buf, size_t cap)
{
    const layer *ol = (net->layers && net->n > 0) ? &net->layers[y2_out_layer(net)] : NULL;
    const tree *t = net->hierarchy;
    if (t && ol && ol->type == SOFTMAX && ol->softmax_tree == t && t->n == ol->outputs) return NULL;
    snprintf(buf, cap, "hierarchical classifiers (softmax tree=) are not implemented on the device for a net.hierarchy that is "
             "not the tree of the output [softmax] layer (n = %d, outputs = %d)", t ? t->n : 0, ol ? ol->outputs : 0);
    return buf;
}

/* The leaf flags are read from the tree at the call: they go up when they differ from what the device holds (the first
 * use, a change_leaves since), which costs one wait; otherwise nothing is copied and nothing waits. */
int y2_hierarchy_leaves(network *net)
{
    y2_engine *e = y2_engine_of(net);
    y2_ldev *d = ld_of(&net->layers[e->out_layer]);
    const tree *t = net->layers[e->out_layer].softmax_tree;
    const size_t bytes = (size_t)t->n * sizeof(int);
    if (d->d_tree_leaf && d->h_tree_leaf && memcmp(d->h_tree_leaf, t->leaf, bytes) == 0) return 0;
    if (!d->h_tree_leaf) d->h_tree_leaf = malloc(bytes);
    if (!d->h_tree_leaf) { y2_fail("out of memory"); return -1; }
    if (!d->d_tree_leaf) HIP_OR_ERR(y2h_malloc((void **)&d->d_tree_leaf, bytes));
    memcpy(d->h_tree_leaf, t->leaf, bytes);
    HIP_OR_ERR(y2h_memcpy_h2d(d->d_tree_leaf, d->h_tree_leaf, bytes, e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    return 0;
}

/* hierarchy_predictions on `nrows` output rows in HBM, on the engine's stream */
int y2_hierarchy_device(network *net, float *rows, int nrows, int only_leaves, const int *d_row_mask)
{
    y2_engine *e = y2_engine_of(net);
    const layer *ol = &net->layers[e->out_layer];
    y2_ldev *d = ld_of(ol);
    const tree *t = ol->softmax_tree;
    if (only_leaves && y2_hierarchy_leaves(net) != 0) return -1;
    HIP_OR_ERR(y2h_hierarchy_rows(rows, ol->outputs, nrows, t->n, d->d_tree_parent, d->d_tree_order, d->d_tree_loff, d->tree_levels,
                                  only_leaves ? d->d_tree_leaf : NULL, d_row_mask, e->stream));
    return 0;
}

int y2_hierarchy_enqueue(network net, int only_leaves)
{
    y2_engine *e = y2_engine_of(&net);
    char why[256];
    const float *rows;
    if (!net.hierarchy) { y2_fail("y2_hierarchy_enqueue: the network has no hierarchy (no [softmax] tree= head)"); return -1; }
    if (y2_hierarchy_refusal(&net, why, sizeof why)) { y2_fail("y2_hierarchy_enqueue: %s", why); return -1; }
    if (!e || !e->built) { y2_fail("y2_hierarchy_enqueue: run a forward first"); return -1; }
    HIP_OR_ERR(y2h_set_device(e->device));
    if (y2_output_device(&net, &rows) != 0) return -1;
    return y2_hierarchy_device(&net, (float *)rows, net.batch, only_leaves, NULL);
}

/* network_predict with hierarchy_predictions(.., only_leaves) between the forward pass and the copy down */
float *y2_predict_hierarchy(network *net, float *input, int only_leaves)
{
    y2_engine *e;
    const float *rows;
    if (y2_prepare(net) != 0) return NULL;
    e = y2_engine_of(net);
    if (y2h_memcpy_h2d(e->d_in_nchw, input, e->in_floats * sizeof(float), e->stream) != 0) { y2_fail("input upload: %s", y2h_last_error()); return NULL; }
    if (y2_engine_forward(net, e->d_in_nchw) != 0 || y2_output_device(net, &rows) != 0) return NULL;
    if (y2_hierarchy_device(net, (float *)rows, net->batch, only_leaves, NULL) != 0) return NULL;
    if (y2_engine_fetch_output(net) != 0) return NULL;
    return e->h_out;
}
