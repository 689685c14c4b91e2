/* pack_index.h -- the index arithmetic of the weight packs, shared by the host packers (pmx_api.hip: pack_weights, pack_wino, pack_conv1), the device
 * packers of the training step (pmx_train.hip) and the tests, which compile it into a stand-alone program.  Plain C; every function is
 * `static inline` and, under hipcc, callable from both sides.  Nothing here touches a weight: only where a weight goes. */
#ifndef PMX_PACK_INDEX_H
#define PMX_PACK_INDEX_H
#include <stddef.h>

#if defined(__HIPCC__)
#define PMX_HD __host__ __device__
#else
#define PMX_HD
#endif

#define PMX_PK_CK 16              /* input channels per chunk of the direct pack */
#define PMX_PK_CAT_C 192          /* channels of the pose network's concat buffer: [feature 128 | PAF 38, 2 pad | heat 19, 5 pad] */
#define PMX_PK_CAT_PAF 128
#define PMX_PK_CAT_HEAT 168

/* output channels of a pack: 64 for up to 64, else the next multiple of 128 */
static inline PMX_HD int pmx_pk_cout_pad(int cout) { return cout <= 64 ? 64 : (cout + 127) / 128 * 128; }

/* OIHW (cout, cin, ks, ks), tap = ky * ks + kx */
static inline PMX_HD size_t pmx_pk_oihw(int n, int ci, int tap, int cin, int T) { return ((size_t)n * cin + ci) * T + tap; }

/* the direct pack [tap][chunk of 16 packed channels][cout_pad][16]: packed input channel k of output channel n */
static inline PMX_HD size_t pmx_pk_direct(int tap, int k, int n, int nch, int cout_pad)
{
    return (((size_t)tap * nch + k / PMX_PK_CK) * cout_pad + n) * PMX_PK_CK + k % PMX_PK_CK;
}

/* Channel maps between the reference's input order and a pack's.  kind 0: identity (k < cin).  kind 1: the 185-input Mconv1_* layers of
 * the pose network -- the reference's F.concat((PAF 38, heat 19, feature 128)) against the concat buffer above.  kind 2 + C: the CPM stages
 * of the face / hand networks -- F.concat((heat C, feature 128)) against [feature 128 | heat C | pad].
 * pmx_pk_ref_of_packed: the reference channel that packed channel k holds, -1 for a pad channel; pmx_pk_packed_of_ref: its inverse. */
static inline PMX_HD int pmx_pk_ref_of_packed(int kind, int k, int cin)
{
    if (kind == 0) return k < cin ? k : -1;
    if (kind == 1)
        return k < PMX_PK_CAT_PAF ? 57 + k : k < PMX_PK_CAT_PAF + 38 ? k - PMX_PK_CAT_PAF
               : k >= PMX_PK_CAT_HEAT && k < PMX_PK_CAT_HEAT + 19 ? 38 + k - PMX_PK_CAT_HEAT : -1;
    { const int C = kind - 2; return k < 128 ? C + k : k < 128 + C ? k - 128 : -1; }
}
static inline PMX_HD int pmx_pk_packed_of_ref(int kind, int ci)
{
    if (kind == 0) return ci;
    if (kind == 1) return ci < 38 ? PMX_PK_CAT_PAF + ci : ci < 57 ? PMX_PK_CAT_HEAT + ci - 38 : ci - 57;
    { const int C = kind - 2; return ci < C ? 128 + ci : ci - C; }
}
/* packed input channels of a layer: cin rounded up to 16, the whole concat buffer for kind 1 */
static inline PMX_HD int pmx_pk_cin_pad(int kind, int cin) { return kind == 1 ? PMX_PK_CAT_C : (cin + PMX_PK_CK - 1) / PMX_PK_CK * PMX_PK_CK; }

/* The layer whose forward is a layer's data gradient (conv_bwd_pack.h), in the direct pack's terms: its input is the layer's g (cout
 * channels, padded with zeros to 64 at least and to a multiple of 16), its outputs are the layer's packed input channels (kind 1: the 192
 * of the concat buffer, else cin), its taps are rotated by 180 degrees. */
static inline PMX_HD int pmx_pk_t_cin_pad(int cout) { return cout < 64 ? 64 : (cout + PMX_PK_CK - 1) / PMX_PK_CK * PMX_PK_CK; }
static inline PMX_HD int pmx_pk_t_cout(int kind, int cin) { return kind == 1 ? PMX_PK_CAT_C : cin; }

/* the Winograd pack [plane][chunk of 32 packed channels][cout_pad / 32][k8-step 4][32][8] */
static inline PMX_HD size_t pmx_pk_wino(int plane, int n, int ci, int nch32, int cout_pad)
{
    return (((((size_t)plane * nch32 + ci / 32) * (cout_pad / 32) + n / 32) * 4 + (ci % 32) / 8) * 32 + n % 32) * 8 + ci % 8;
}
static inline PMX_HD int pmx_pk_wino_planes(int ks) { return ks == 3 ? 16 : 81; }

/* conv1_1's fused-kernel pack [channel half 2][k-pair 14][k of the pair 2][channel 32], k = tap * 3 + input channel: the float of conv1_1's
 * direct pack [tap 9][1 chunk][cout_pad][16] that position idx holds, -1 for the 28th k of a channel (a zero) */
#define PMX_PK_CONV1_FLOATS (2 * 14 * 2 * 32)
static inline PMX_HD long long pmx_pk_conv1_src(int idx, int cout_pad)
{
    const int n = idx % 32, kk = (idx / 32) % 2, sp = (idx / 64) % 14, hf = idx / 896, k = 2 * sp + kk;
    return k < 27 ? (long long)pmx_pk_direct(k / 3, k % 3, hf * 32 + n, 1, cout_pad) : -1;
}
#endif
