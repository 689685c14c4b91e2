/* wgrad_strips.h -- how the weight-gradient kernels (conv_bwd.hip) cut the B * H image rows of a layer into strips.  Plain C, shared by the
 * library and by the stand-alone program of the tests (tests/trunk_strips_main.c); the rules themselves: include/pose_mi355x.h
 * (pmx_conv2d_backward, pmx_backward_trunk).  Every constant here is independent of the device: the strips fix the summation order. */
#ifndef PMX_WGRAD_STRIPS_H
#define PMX_WGRAD_STRIPS_H

#define PMX_WGRAD_WAVES 2048 /* 256 CUs x 4 SIMDs x 2 */

/* the units of one strip of the generic kernel: (tap row, 32 co, NCI x 32 ci), NCI = 1 / 2 / 4 for 7x7 / 3x3 / 1x1; one wave each */
static inline int pmx_wgrad_nci(int ks) { return ks == 7 ? 1 : ks == 3 ? 2 : 4; }
static inline int pmx_wgrad_units(int cg, int cx, int ks)
{
    const int nci = cx / 32, per = pmx_wgrad_nci(ks);
    return (nci + per - 1) / per * ks * (cg / 32);
}

/* s0 requested strips, at most `cap` and at most one per row -> S strips of *rows rows.  rows = ceil(total / s0) gives S <= s0 (the head
 * chain and pmx_conv2d_backward); round_down: rows = floor(total / s0) gives s0 <= S < 2 * s0, so a rule that asks for the strips that
 * make PMX_WGRAD_WAVES waves gets at least that many (the trunk chain) */
static inline int pmx_wgrad_cut(long long total, long long s0, long long cap, int round_down, int* rows)
{
    long long r;
    if (s0 > cap) s0 = cap;
    if (s0 > total) s0 = total;
    if (s0 < 1) s0 = 1;
    r = round_down ? total / s0 : (total + s0 - 1) / s0;
    *rows = (int)r;
    return (int)((total + r - 1) / r);
}

/* the generic kernel: as many strips as give every SIMD of an MI355X two waves, at most `cap` (cg / cx: cout / cin rounded up to 32) */
static inline int pmx_wgrad_strips_cap(int B, int H, int cg, int cx, int ks, int forced, int cap, int round_down, int* rows)
{
    long long s0 = forced;
    if (s0 <= 0) {
        const long long units = pmx_wgrad_units(cg, cx, ks);
        s0 = (PMX_WGRAD_WAVES + units - 1) / units;
    }
    return pmx_wgrad_cut((long long)B * H, s0, cap, round_down, rows);
}

/* the f16 kernel (conv_wgrad_f16.hip; option "grad_precision" = 2).  A block of four waves owns (tap row, 4 x 32 co, NCI x 32 ci), NCI = 1 / 2
 * for 7x7 / 3x3.  Every image row is cut into ceil(W / 16) GROUPS of 16 consecutive pixels, the last one padded with zero operands; an
 * accumulator sees one MFMA per group, the groups of a row left to right, the rows of its strip top to bottom.  The strips: as many as
 * give PMX_WGRAD_F16_WAVES waves, R = ceil(B * H / S0) rows each, as the fp32 rule. */
#define PMX_WGRAD_F16_WAVES 4096 /* 256 CUs x 4 SIMDs x 4: measured, EXPERIMENTS.md E54 */
static inline int pmx_wgrad_f16_nci(int ks) { return ks == 7 ? 1 : 2; }
static inline int pmx_wgrad_f16_blocks(int cg, int cx, int ks)
{
    const int per = pmx_wgrad_f16_nci(ks);
    return (cg / 32 + 3) / 4 * ks * ((cx / 32 + per - 1) / per);
}
static inline int pmx_wgrad_f16_groups(int W) { return (W + 15) / 16; }
static inline int pmx_wgrad_f16_strips(int B, int H, int cg, int cx, int ks, int forced, int cap, int* rows)
{
    long long s0 = forced;
    if (s0 <= 0) {
        const long long waves = 4ll * pmx_wgrad_f16_blocks(cg, cx, ks);
        s0 = (PMX_WGRAD_F16_WAVES + waves - 1) / waves;
    }
    return pmx_wgrad_cut((long long)B * H, s0, cap, 0, rows);
}

/* conv1_1's kernel: one wave per strip, `cap` (PMX_WGRAD_CONV1_STRIPS = PMX_WGRAD_WAVES) strips asked for, rows rounded down: at least
 * PMX_WGRAD_WAVES strips whenever B * H >= PMX_WGRAD_WAVES, fewer than twice as many */
static inline int pmx_wgrad_conv1_strips(int B, int H, int forced, int cap, int* rows)
{
    return pmx_wgrad_cut((long long)B * H, forced > 0 ? forced : cap, cap, 1, rows);
}

#endif
