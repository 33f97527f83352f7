/* prints the layout of y2h_rec_args (include/y2_hip.h) for tests/test_rec_rule_host.py, which holds the ctypes mirror in
 * sr_object_detection_amd/darknet.py against it */
#include <stddef.h>
#include <stdio.h>
#include "y2_hip.h"
#define F(f) printf("%s %zu\n", #f, offsetof(y2h_rec_args, f));
int main(void)
{
    printf("sizeof %zu\n", sizeof(y2h_rec_args));
    F(x) F(w) F(bias) F(mean) F(scale) F(rinv) F(bn) F(act) F(pre) F(rows) F(k) F(n) F(h) F(mode) F(shortcut) F(proj)
    F(state) F(out) F(out2) F(z) F(xcopy)
    printf("enums %d %d %d %d %d %d %d\n", Y2H_REC_DENSE, Y2H_REC_RNN, Y2H_REC_GRU_ZR, Y2H_REC_GRU_H, Y2H_REC_REF,
           Y2H_REC_SKINNY, Y2H_REC_SKINNY_MAX_ROWS);
    return 0;
}
