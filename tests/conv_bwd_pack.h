/* conv_bwd_pack.h -- the layer whose FORWARD is a convolution's data gradient, as an independent host restatement of the library's transposed
 * pack (csrc/pack_index.h::pmx_pk_transposed_value): the tests' stand-alone programs compile it.  Plain C. */
#ifndef PMX_CONV_BWD_PACK_H
#define PMX_CONV_BWD_PACK_H
#include <stddef.h>

/* wt[ci][co][ky][kx] = w[co][ci][ks-1-ky][ks-1-kx]: OIHW (cout, cin, ks, ks) -> OIHW (cin, cout, ks, ks), transposed and rotated by 180
 * degrees.  A stride-1 convolution of g with wt, padded by ks/2, is the gradient of the convolution with w at its input. */
static inline void pmx_conv_flip_weights(const float* w, int cout, int cin, int ks, float* wt)
{
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int ky = 0; ky < ks; ++ky)
                for (int kx = 0; kx < ks; ++kx)
                    wt[(((size_t)ci * cout + co) * ks + ky) * ks + kx] = w[(((size_t)co * cin + ci) * ks + (ks - 1 - ky)) * ks + (ks - 1 - kx)];
}

/* The same layer for a convolution whose input is read from a buffer in ANOTHER channel order (Mconv1_*: the concat buffer), so that its data
 * gradient comes out in the buffer's order: wt[k][co][ky][kx] = w[co][map[k]][ks-1-ky][ks-1-kx] for the nmap buffer channels k, map[k] = the
 * input channel of w that buffer channel k holds, or -1 for a pad channel, whose nmap-th row is all +0.0f.  wt: OIHW (nmap, cout, ks, ks). */
static inline void pmx_conv_flip_weights_mapped(const float* w, int cout, int cin, int ks, const int* map, int nmap, float* wt)
{
    for (int k = 0; k < nmap; ++k)
        for (int co = 0; co < cout; ++co)
            for (int ky = 0; ky < ks; ++ky)
                for (int kx = 0; kx < ks; ++kx)
                    wt[(((size_t)k * cout + co) * ks + ky) * ks + kx] =
                        map[k] >= 0 && map[k] < cin ? w[(((size_t)co * cin + map[k]) * ks + (ks - 1 - ky)) * ks + (ks - 1 - kx)] : 0.0f;
}
#endif
