/* Stand-alone program of tests/test_train_full_host.py: csrc/pack_index.h's pmx_pk_conv1_src -- where every float of conv1_1's
 * fused-kernel pack [half 2][k-pair 14][k 2][32] comes from in the direct pack [tap 9][1 chunk][cout_pad][16] -- over all positions.
 * usage: conv1_pack_main <cout_pad>; prints one line "idx src" per position (src -1: the zero 28th k). */
#include <stdio.h>
#include <stdlib.h>
#include "pack_index.h"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    const int cout_pad = atoi(argv[1]);
    const long long direct = 9LL * cout_pad * PMX_PK_CK;
    float* pack = (float*)malloc((size_t)direct * sizeof(float));      /* the sanitizer sees every index used */
    if (!pack) return 3;
    for (long long i = 0; i < direct; ++i) pack[i] = (float)i;
    for (int idx = 0; idx < PMX_PK_CONV1_FLOATS; ++idx) {
        const long long src = pmx_pk_conv1_src(idx, cout_pad);
        if (src >= direct) return 4;
        printf("%d %lld %.0f\n", idx, src, src >= 0 ? pack[src] : -1.0);
    }
    free(pack);
    return 0;
}
