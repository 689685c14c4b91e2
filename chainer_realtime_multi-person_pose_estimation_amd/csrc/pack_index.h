/* pack_index.h -- the definition of every weight pack: where a weight goes (the index functions) and, per element of a pack, what it holds
 * as a function of the pack's source (the value functions at the end).  The device packers (pmx_packs.hip) are `dst[idx] = value(idx)` over
 * these; the tests compile the header into a stand-alone host program.  Plain C; every function is `static inline` and, under hipcc,
 * callable from both sides (PMX_HD, f16_round.h). */
#ifndef PMX_PACK_INDEX_H
#define PMX_PACK_INDEX_H
#include <stddef.h>

#include "f16_round.h"

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

/* The layer whose forward is a layer's data gradient (pmx_pk_transposed_value), in the direct pack's terms: its input is the layer's g (cout
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

/* ---- the value of element idx of every pack ----------------------------------------------------------------------------------------------
 * One evaluation per element of the pack (a float; a uint16 of the f16 and bf16x3 packs), so the pad positions are written (+0) like
 * everything else.  A PackJob names one pack to write: a step's table-driven launch gives a job the blocks [blk0, next blk0), 256 elements
 * of its pack each; a one-off build is a single job. */
typedef struct { int cout, cin, T, kind, nch, cout_pad; } PackGeo;      /* of the pack WRITTEN (nch chunks of 16 packed input channels) */
typedef struct {
    const float* src;      /* direct / transposed: the layer's master weights (w OIHW | b); every other pack: the direct pack it derives from */
    void* dst;             /* float; f16 / bf16x3: uint16_t */
    float* bias;           /* direct: the padded bias */
    PackGeo p;
    int t_cout, ks;        /* transposed: output channels of the transposed layer; Winograd: the kernel size */
    unsigned total, blk0;  /* elements of the pack, first block of the job in the launch */
} PackJob;

/* master (w OIHW | b) -> the layer's direct pack and its padded bias (idx < cout_pad) */
static inline PMX_HD float pmx_pk_direct_value(const PackJob* j, unsigned idx)
{
    const PackGeo p = j->p;
    const int c = idx % PMX_PK_CK, n = (idx / PMX_PK_CK) % p.cout_pad;
    const unsigned pc = idx / PMX_PK_CK / p.cout_pad;
    const int ch = pc % p.nch, tap = pc / p.nch, k = ch * PMX_PK_CK + c;
    const int src = pmx_pk_ref_of_packed(p.kind, k, p.cin);
    return src >= 0 && n < p.cout ? j->src[pmx_pk_oihw(n, src, tap, p.cin, p.T)] : 0.0f;
}
static inline PMX_HD float pmx_pk_bias_value(const PackJob* j, unsigned idx)
{
    return idx < (unsigned)j->p.cout ? j->src[(size_t)j->p.cout * j->p.cin * j->p.T + idx] : 0.0f;
}

/* master w -> the direct pack of the layer whose forward is the data gradient: output channel n = the layer's packed input channel, input
 * channel k = the layer's output channel (the zero-padded g), taps rotated by 180 degrees.  p describes the LAYER (cout, cin, T, kind);
 * nch / cout_pad the transposed pack. */
static inline PMX_HD float pmx_pk_transposed_value(const PackJob* j, unsigned idx)
{
    const PackGeo p = j->p;
    const int c = idx % PMX_PK_CK, n = (idx / PMX_PK_CK) % p.cout_pad;
    const unsigned pc = idx / PMX_PK_CK / p.cout_pad;
    const int ch = pc % p.nch, tap = pc / p.nch, k = ch * PMX_PK_CK + c;
    const int src = n < j->t_cout ? pmx_pk_ref_of_packed(p.kind, n, p.cin) : -1;
    return src >= 0 && k < p.cout ? j->src[pmx_pk_oihw(k, src, p.T - 1 - tap, p.cin, p.T)] : 0.0f;
}

/* direct pack -> Winograd F(2x2, 3x3) pack: U = G g G^T per (cout, cin), G = [[1,0,0],[1/2,1/2,1/2],[1/2,-1/2,1/2],[0,0,1]], evaluated in
 * double, each row and then each column as (G0 a + G1 b) + G2 c, and rounded once to fp32 (oracle/conv_fma_ref.c::conv_wino_ref does the
 * same; the unit that evaluates this must not contract a multiply and an add).  plane = sub-kernel * 16 + 4i + j.  ks = 3: one sub-kernel;
 * ks = 7: four, sub-kernel (sy, sx) = taps (3 sy .. 3 sy + 2, 3 sx .. 3 sx + 2); row 6 and column 6 of the 7x7 kernel are two 1x3 / two 3x1
 * sub-kernels with the 1-D transform G g (planes 64 .., 72 ..), tap (6, 6) is plane 80.  The four k8-steps of a wave's 32 channels lie
 * 1 KB apart (an immediate offset of the kernel's load). */
static inline PMX_HD float pmx_pk_wino_value(const PackJob* j, unsigned idx)
{
    const float* wp = j->src;
    const int ks = j->ks, nch16 = j->p.nch, cout_pad = j->p.cout_pad;
    const int nch32 = nch16 * PMX_PK_CK / 32, nb32 = cout_pad / 32;
    const int ci8 = idx % 8, n32 = (idx / 8) % 32, k8 = (idx / 256) % 4, nb = (idx / 1024) % nb32;
    const unsigned pc = idx / 1024 / nb32;
    const int c32 = pc % nch32, plane = pc / nch32;
    const int n = nb * 32 + n32, ci = c32 * 32 + k8 * 8 + ci8;
    const double Gm[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
#define PMX_PK_TAPW(ky, kx) ((double)wp[pmx_pk_direct((ky) * ks + (kx), ci, n, nch16, cout_pad)])
    double val;
    if (plane < 64) {
        const int sub = plane / 16, i = (plane % 16) / 4, jj = plane % 4;
        double gg[3];
        for (int kx = 0; kx < 3; ++kx)
            gg[kx] = (Gm[i][0] * PMX_PK_TAPW(3 * (sub >> 1) + 0, 3 * (sub & 1) + kx) + Gm[i][1] * PMX_PK_TAPW(3 * (sub >> 1) + 1, 3 * (sub & 1) + kx)) +
                     Gm[i][2] * PMX_PK_TAPW(3 * (sub >> 1) + 2, 3 * (sub & 1) + kx);
        val = (gg[0] * Gm[jj][0] + gg[1] * Gm[jj][1]) + gg[2] * Gm[jj][2];
    } else if (plane < 72) {
        const int sub = (plane - 64) / 4, f = (plane - 64) % 4;
        val = (Gm[f][0] * PMX_PK_TAPW(6, 3 * sub + 0) + Gm[f][1] * PMX_PK_TAPW(6, 3 * sub + 1)) + Gm[f][2] * PMX_PK_TAPW(6, 3 * sub + 2);
    } else if (plane < 80) {
        const int sub = (plane - 72) / 4, f = (plane - 72) % 4;
        val = (Gm[f][0] * PMX_PK_TAPW(3 * sub + 0, 6) + Gm[f][1] * PMX_PK_TAPW(3 * sub + 1, 6)) + Gm[f][2] * PMX_PK_TAPW(3 * sub + 2, 6);
    } else val = PMX_PK_TAPW(6, 6);
#undef PMX_PK_TAPW
    return (float)val;
}

/* direct pack -> f16 pack, the direct pack's own layout [tap][chunk][cout_pad][16] (so the concat channel map comes along) */
static inline PMX_HD uint16_t pmx_pk_f16_value(const PackJob* j, unsigned idx) { return f16_rn_sat(j->src[idx]); }

/* fp32 -> bf16 bits, round-to-nearest-even (a NaN stays one: | 0x40), and back */
static inline PMX_HD uint16_t bf16_rn(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
static inline PMX_HD float bf16_f(uint16_t h)
{
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
/* direct pack -> bf16x3 pack [tap][chunk][plane hi|mid|lo][cout_pad][16]: three bf16 terms of every weight, each the rounding of what the
 * terms before it leave (fp32 subtractions), as conv_bf16x3_kernel splits the activations */
static inline PMX_HD uint16_t pmx_pk_bf16x3_value(const PackJob* j, unsigned idx)
{
    const unsigned k = idx % PMX_PK_CK, n = (idx / PMX_PK_CK) % j->p.cout_pad;
    const unsigned pp = idx / PMX_PK_CK / j->p.cout_pad, plane = pp % 3, pc = pp / 3;
    const float x = j->src[((size_t)pc * j->p.cout_pad + n) * PMX_PK_CK + k];
    const uint16_t h = bf16_rn(x);
    if (plane == 0) return h;
    { const float r1 = x - bf16_f(h);
      const uint16_t m = bf16_rn(r1);
      return plane == 1 ? m : bf16_rn(r1 - bf16_f(m)); }
}

/* conv1_1's direct pack -> its fused-kernel pack (the 28th k of every channel: +0.0f) */
static inline PMX_HD float pmx_pk_conv1_value(const PackJob* j, unsigned idx)
{
    const long long src = pmx_pk_conv1_src((int)idx, j->p.cout_pad);
    return src >= 0 ? j->src[src] : 0.0f;
}

/* a layer's direct pack dw and padded bias db -> float i of (w OIHW, reference input order | b) */
static inline PMX_HD float pmx_pk_unpack_value(const float* dw, const float* db, PackGeo p, unsigned i)
{
    const unsigned nw = (unsigned)p.cout * p.cin * p.T;
    if (i >= nw) return db[i - nw];
    { const int tap = i % p.T, src = (i / p.T) % p.cin, n = i / p.T / p.cin;
      return dw[pmx_pk_direct(tap, pmx_pk_packed_of_ref(p.kind, src), n, p.nch, p.cout_pad)]; }
}
#endif
