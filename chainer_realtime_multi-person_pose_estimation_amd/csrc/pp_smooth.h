// pp_smooth.h -- the smoothed-heat-map tile of the post-process's fast path, shared by postproc.hip (pp_peaks_fast_kernel: NMS + peaks,
// and the smoothing of pmx_keypoints) and pmx_boxes.hip (per-tile arg-max records of pmx_keypoints_images): ONE text of the arithmetic per
// smoothed value, so both produce the same bits.  Include after pmx_common.h; the includer compiles with -ffp-contract=off.
#pragma once
#include "pmx_common.h"

#pragma clang fp contract(off)

#define PK_TS 32                                   // NMS output tile (pixels)
#define PK_UW_MAX (PK_TS + 2 + 2 * PMX_GAUSS_MAX_RADIUS)   // 66
#define PK_US (PK_UW_MAX + 1)                      // LDS row stride (floats)

// scipy 'reflect' (d c b a | a b c d), any distance
__device__ __forceinline__ int reflect_idx(int i, int n)
{
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

// ------------------------------------------------------------------------------------------ peaks (fast path)
// Same arithmetic as pp_peaks_kernel, specialised for a compile-time Gaussian radius R (10 for sigma 2.5):
//   * the tile's row / column resize tables (corner indices, float64 weights, reflect applied) are staged in LDS once,
//     so a bilinear sample costs 4 map loads instead of 4 + 12 table loads from global memory;
//   * both 1-D passes use a sliding window: a thread produces SEG consecutive outputs of one column (row) from
//     SEG + 2R LDS reads held in registers instead of 2R + 1 reads per output.
// The float32 / float64 operation order per output is unchanged (SciPy's: centre tap, then pairs from the outermost
// inwards), so the results are bit-identical to the generic kernel (tests compare both against the oracle).
//
// The tile as two macros, so that pp_peaks_fast_kernel expands to exactly the tokens it was written with (a device function or a
// lambda changes its machine code: tools/code_object_diff.py):
//   PP_SMOOTH_FAST_DECL(R)  constants and LDS arrays of the tile (at the top of the kernel);
//   PP_SMOOTH_FAST_BODY(R)  with `tid`, `b`, `ch`, `y0`, `x0` and maps / tab / buf / map_h / map_w / keep_smoothed / n_ch / do_nms in scope:
//                           leaves sS[(r + 1) * SW + (c + 1)] = smoothed(y0 + r, x0 + c), r, c in [-1, PK_TS] (0 outside the map), after
//                           a block barrier.  RETURNS from the kernel when do_nms && !keep_smoothed and the patch maximum rules out a peak.

#define PP_SMOOTH_FAST_DECL(R) \
    constexpr int UW = PK_TS + 2 + 2 * R;   /* 54 */                                                   \
    constexpr int US = UW + 1;                                                                         \
    constexpr int VR = PK_TS + 2;   /* 34 rows/cols that feed the NMS */                               \
    constexpr int SEG = 9;   /* outputs per thread and pass */                                         \
    constexpr int NSEG = (VR + SEG - 1) / SEG;   /* 4 */                                               \
    constexpr int SW = PK_TS + 3;                                                                      \
    __shared__ float sU[UW * US];                                                                      \
    __shared__ float sV[VR * US];                                                                      \
    __shared__ float sS[VR * SW];                                                                      \
    __shared__ double sG[2 * R + 1];                                                                   \
    __shared__ double sYlo[UW], sYhi[UW], sXlo[UW], sXhi[UW];                                          \
    __shared__ int sY0[UW], sY1[UW], sX0[UW], sX1[UW];                                                 \
    constexpr int PW = 56;   /* low-resolution patch staged in LDS (rows x cols), covers in == out */  \
    __shared__ float sP[PW * PW];                                                                      \
    __shared__ int sBox[4];   /* patch origin (row, col) and extent */                                 \
    __shared__ float sPmax[4];   /* per-wave maximum of the patch (threshold pruning) */               \


#define PP_SMOOTH_FAST_BODY(R) \
    if (tid < 2 * R + 1) sG[tid] = tab.gauss[tid];                                                                                              \
    if (tid < UW) {                                                                                                                             \
        const int gy = reflect_idx(y0 - 1 - R + tid, map_h);                                                                                    \
        sY0[tid] = tab.yi0[gy]; sY1[tid] = tab.yi1[gy]; sYlo[tid] = tab.ylo[gy]; sYhi[tid] = tab.yhi[gy];                                       \
    } else if (tid >= 64 && tid < 64 + UW) {                                                                                                    \
        const int k = tid - 64;                                                                                                                 \
        const int gx = reflect_idx(x0 - 1 - R + k, map_w);                                                                                      \
        sX0[k] = tab.xi0[gx]; sX1[k] = tab.xi1[gx]; sXlo[k] = tab.xlo[gx]; sXhi[k] = tab.xhi[gx];                                               \
    }                                                                                                                                           \
    __syncthreads();                                                                                                                            \
                                                                                                                                                \
    const float* base = maps.heat + (long long)b * maps.sbh + (long long)ch * maps.sc;                                                          \
    /* bounding box of the low-resolution pixels this tile samples (a 7x upsampled tile touches ~10 x 10 of them): */                           \
    /* stage it in LDS once instead of 4 scattered global loads per full-resolution sample */                                                   \
    if (tid < 64) {                                                                                                                             \
        int lo_y = 1 << 30, hi_y = -1, lo_x = 1 << 30, hi_x = -1;                                                                               \
        if (tid < UW) { lo_y = sY0[tid]; hi_y = sY1[tid]; lo_x = sX0[tid]; hi_x = sX1[tid]; }                                                   \
_Pragma("unroll")                                                                                                                               \
        for (int off = 32; off >= 1; off >>= 1) {                                                                                               \
            lo_y = min(lo_y, __shfl_xor(lo_y, off)); hi_y = max(hi_y, __shfl_xor(hi_y, off));                                                   \
            lo_x = min(lo_x, __shfl_xor(lo_x, off)); hi_x = max(hi_x, __shfl_xor(hi_x, off));                                                   \
        }                                                                                                                                       \
        if (tid == 0) { sBox[0] = lo_y; sBox[1] = lo_x; sBox[2] = hi_y - lo_y + 1; sBox[3] = hi_x - lo_x + 1; }                                 \
    }                                                                                                                                           \
    __syncthreads();                                                                                                                            \
    const int py0 = sBox[0], px0 = sBox[1], ph = sBox[2], pw = sBox[3];                                                                         \
    const bool patched = ph <= PW && pw <= PW;   /* block-uniform */                                                                            \
    if (patched) {                                                                                                                              \
        float pmax = -3.0e38f;                                                                                                                  \
        for (int i = tid; i < ph * pw; i += 256) {                                                                                              \
            const int r = i / pw, c = i - r * pw;                                                                                               \
            const float v = base[(long long)(py0 + r) * maps.sy + (long long)(px0 + c) * maps.sx];                                              \
            sP[r * PW + c] = v;                                                                                                                 \
            pmax = fmaxf(pmax, v);                                                                                                              \
        }                                                                                                                                       \
        /* Threshold pruning.  Every smoothed value of this tile is a convex combination (bilinear weights, then Gaussian taps: all */          \
        /* non-negative, each set summing to 1 up to rounding) of the low-resolution pixels of the patch, so it cannot exceed their maximum */  \
        /* by more than rounding noise; a peak needs smoothed > 0.05 (pose_detector.py:97).  If the patch maximum is below the threshold */     \
        /* with a 1e-5 relative safety margin (the rounded weight sums exceed 1 by < 1e-6), no pixel of the tile can be a peak: skip the */     \
        /* two float64 passes and the NMS.  Results are unchanged by construction (real heat maps are ~0 away from the joints: most */          \
        /* tiles take this exit).  Not taken when the smoothed map itself is wanted (keep_smoothed, key-point nets). */                         \
        if (do_nms && !keep_smoothed) {                                                                                                         \
_Pragma("unroll")                                                                                                                               \
            for (int off = 32; off >= 1; off >>= 1) pmax = fmaxf(pmax, __shfl_xor(pmax, off));                                                  \
            if ((tid & 63) == 0) sPmax[tid >> 6] = pmax;                                                                                        \
        }                                                                                                                                       \
        __syncthreads();                                                                                                                        \
        if (do_nms && !keep_smoothed) {                                                                                                         \
            const float m = fmaxf(fmaxf(sPmax[0], sPmax[1]), fmaxf(sPmax[2], sPmax[3]));                                                        \
            if (m * 1.00001f < PMX_HEATMAP_PEAK_THRESH && m < PMX_HEATMAP_PEAK_THRESH) return;   /* block-uniform */                            \
        }                                                                                                                                       \
    }                                                                                                                                           \
    for (int i = tid; i < UW * UW; i += 256) {                                                                                                  \
        const int ur = i / UW, uc = i - ur * UW;                                                                                                \
        const double ylo = sYlo[ur], yhi = sYhi[ur], xlo = sXlo[uc], xhi = sXhi[uc];                                                            \
        const float w1 = (float)(ylo * xlo), w2 = (float)(ylo * xhi), w3 = (float)(yhi * xlo), w4 = (float)(yhi * xhi);                         \
        float x00, x01, x10, x11;                                                                                                               \
        if (patched) {                                                                                                                          \
            const int r0 = (sY0[ur] - py0) * PW, r1 = (sY1[ur] - py0) * PW, c0 = sX0[uc] - px0, c1 = sX1[uc] - px0;                             \
            x00 = sP[r0 + c0]; x01 = sP[r0 + c1]; x10 = sP[r1 + c0]; x11 = sP[r1 + c1];                                                         \
        } else {                                                                                                                                \
            const long long r0 = sY0[ur] * maps.sy, r1 = sY1[ur] * maps.sy, c0 = sX0[uc] * maps.sx, c1 = sX1[uc] * maps.sx;                     \
            x00 = base[r0 + c0]; x01 = base[r0 + c1]; x10 = base[r1 + c0]; x11 = base[r1 + c1];                                                 \
        }                                                                                                                                       \
        float v = w1 * x00;                                                                                                                     \
        v = v + w2 * x01;                                                                                                                       \
        v = v + w3 * x10;                                                                                                                       \
        v = v + w4 * x11;                                                                                                                       \
        sU[ur * US + uc] = v;                                                                                                                   \
    }                                                                                                                                           \
    __syncthreads();                                                                                                                            \
                                                                                                                                                \
    /* axis-0 pass: thread = (column, segment of SEG rows) */                                                                                   \
    for (int i = tid; i < UW * NSEG; i += 256) {                                                                                                \
        const int vc = i % UW, sg = i / UW;                                                                                                     \
        const int r0 = sg * SEG;                                                                                                                \
        float win[SEG + 2 * R];                                                                                                                 \
_Pragma("unroll")                                                                                                                               \
        for (int k = 0; k < SEG + 2 * R; ++k) win[k] = (r0 + k < UW) ? sU[(r0 + k) * US + vc] : 0.f;                                            \
_Pragma("unroll")                                                                                                                               \
        for (int o = 0; o < SEG; ++o) {                                                                                                         \
            if (r0 + o < VR) {                                                                                                                  \
                double acc = (double)win[o + R] * sG[R];                                                                                        \
_Pragma("unroll")                                                                                                                               \
                for (int j = R; j >= 1; --j) acc = acc + ((double)win[o + R - j] + (double)win[o + R + j]) * sG[R - j];                         \
                sV[(r0 + o) * US + vc] = (float)acc;                                                                                            \
            }                                                                                                                                   \
        }                                                                                                                                       \
    }                                                                                                                                           \
    __syncthreads();                                                                                                                            \
                                                                                                                                                \
    /* axis-1 pass: thread = (row, segment of SEG columns); positions outside the map are the NMS zero padding */                               \
    for (int i = tid; i < VR * NSEG; i += 256) {                                                                                                \
        const int sr = i % VR, sg = i / VR;                                                                                                     \
        const int c0 = sg * SEG;                                                                                                                \
        const int y = y0 - 1 + sr;                                                                                                              \
        float win[SEG + 2 * R];                                                                                                                 \
_Pragma("unroll")                                                                                                                               \
        for (int k = 0; k < SEG + 2 * R; ++k) win[k] = (c0 + k < UW) ? sV[sr * US + c0 + k] : 0.f;                                              \
_Pragma("unroll")                                                                                                                               \
        for (int o = 0; o < SEG; ++o) {                                                                                                         \
            const int sc = c0 + o;                                                                                                              \
            if (sc < VR) {                                                                                                                      \
                const int x = x0 - 1 + sc;                                                                                                      \
                float out = 0.f;                                                                                                                \
                if (y >= 0 && y < map_h && x >= 0 && x < map_w) {                                                                               \
                    double acc = (double)win[o + R] * sG[R];                                                                                    \
_Pragma("unroll")                                                                                                                               \
                    for (int j = R; j >= 1; --j) acc = acc + ((double)win[o + R - j] + (double)win[o + R + j]) * sG[R - j];                     \
                    out = (float)acc;                                                                                                           \
                    if (keep_smoothed && sr >= 1 && sr <= PK_TS && sc >= 1 && sc <= PK_TS)                                                      \
                        buf.smoothed[(((long long)b * n_ch + ch) * map_h + y) * map_w + x] = out;                                               \
                }                                                                                                                               \
                sS[sr * SW + sc] = out;                                                                                                         \
            }                                                                                                                                   \
        }                                                                                                                                       \
    }                                                                                                                                           \
    __syncthreads();

// Per-channel arg-max of the key-point nets (postproc.hip::pp_argmax_kernel, pmx_boxes.hip): the reference's
// `np.where(heatmap == max_value)` needs the maximum, its multiplicity and the two smallest row-major indices.  The merge is exact,
// commutative and associative: partial records of any partition of a map merge to the record of the whole map.
// NaN: `heatmap.max()` of a map that holds a NaN anywhere is NaN, `max_value > thresh` is then false and the key point is None.  A plain
// '>' / '==' scan skips a NaN, so the scans call argmax_take, which turns the record into the one NaN record (argmax_nan: the same bits
// whatever the NaN's payload and wherever it was met), and the merge lets that record absorb any other: still exact, commutative and
// associative.
struct ArgMax { float v; int cnt; int i0; int i1; };   // max value, multiplicity, two smallest row-major indices (16 bytes)

__device__ __forceinline__ ArgMax argmax_nan()
{
    ArgMax r;
    r.v = __builtin_nanf(""); r.cnt = 0; r.i0 = 0x7fffffff; r.i1 = 0x7fffffff;
    return r;
}

// one more value of a scan whose indices are unique (ascending or not)
__device__ __forceinline__ void argmax_take(ArgMax& a, float v, int idx)
{
    if (v != v || a.v != a.v) { a = argmax_nan(); return; }
    if (v > a.v) { a.v = v; a.cnt = 1; a.i0 = idx; a.i1 = 0x7fffffff; }
    else if (v == a.v) {
        a.cnt += 1;
        if (idx < a.i0) { a.i1 = a.i0; a.i0 = idx; } else if (idx < a.i1) a.i1 = idx;
    }
}

__device__ __forceinline__ ArgMax argmax_merge(const ArgMax& a, const ArgMax& b)
{
    if (a.v != a.v || b.v != b.v) return argmax_nan();
    if (a.v > b.v) return a;
    if (b.v > a.v) return b;
    ArgMax r;
    r.v = a.v;
    r.cnt = a.cnt + b.cnt;
    // two smallest of {a.i0, a.i1, b.i0, b.i1} (INT_MAX = empty)
    const int lo = min(a.i0, b.i0), hi = max(a.i0, b.i0);
    r.i0 = lo;
    r.i1 = min(hi, min(a.i1, b.i1));
    return r;
}
