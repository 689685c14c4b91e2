// conv_bwd.hip -- the launches of pmx_conv2d_backward that are not the dispatcher's: the mask kernel (g from dy and z), the bias gradient
// and the weight gradient.  Semantics and the summation orders: include/pose_mi355x.h (pmx_conv2d_backward); tiling: DESIGN.md 4.7.
//
//   weight gradient  per tap (ky, kx) a GEMM  dw[co][ci] = sum over pixels p of g[p][co] * x[p + (ky-pad, kx-pad)][ci]:  M = cout, N = cin,
//                    K = B * H * W.  NHWC puts the channels of a pixel side by side, which is the operand layout of v_mfma_f32_32x32x2_f32
//                    as it stands: A = 32 consecutive co of pixel p (lanes 0-31) and of pixel p + 1 (lanes 32-63), B = 32 consecutive ci of
//                    the two tap-shifted pixels; each lane loads ONE float per operand, a half-wave reads one 128-byte run.
//                    A wave owns one UNIT = (tap row ky, 32 co, NCI x 32 ci) and keeps the KS taps of the row for NCI ci tiles in
//                    NCI x KS accumulators (7x7: 7 x 16 registers; 3x3: 2 x 3; 1x1: 4 x 1), so a g fragment feeds NCI * KS MFMAs and an x
//                    fragment is fetched once per (pixel pair, kx).  The four waves of a block are four consecutive units: they differ in
//                    the co tile (or the tap row) and read the same x pixels, which the vector L1 serves.  The operands are NOT staged in
//                    LDS: one dword per lane per MFMA is 4 bytes / lane / 64 cycles, far below what the L1 delivers, and a tap outside
//                    the image is a select on the loaded value, not a halo.
//                    K is cut into strips of image rows (blockIdx.y); a strip's accumulators go to its own slot [strip][tap][co][ci] of the
//                    workspace and conv_wgrad_combine_kernel adds the slots left to right and writes OIHW.  No atomics.
//   order            an accumulator element sees fmaf(g, x, acc) for the pixels of its strip in row-major order: the MFMA adds its two K
//                    slots in order (pixel p, then p + 1) and consecutive MFMAs of an accumulator are consecutive pixel pairs.
#include "pmx_ctx.h"
#include "wgrad_strips.h"
#include "f16_round.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct WgradArgs {
    const float* g; const float* x; float* ws;
    int H, W, cg, cx, nco, nci, n_units, rows;      // nco / nci: 32-channel tiles of g / x; rows: image rows per strip
    int ldg, ldx;                                   // floats per pixel of g / x (>= cg / cx: the operands may be slices of wider buffers)
    long long total_rows;                           // B * H
};

template <int KS, int NCI>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) conv_wgrad_kernel(WgradArgs a)      // (two waves per SIMD hide the loads' latency)
{
    constexpr int PAD = KS / 2;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5, l = lane & 31;
    const int unit = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);       // (wave-uniform, and the compiler is told so)
    if (unit >= a.n_units) return;                  // (no barrier anywhere below: a wave may leave alone)
    const int co_t = unit % a.nco, ky = (unit / a.nco) % KS, cig = unit / (a.nco * KS);
    const long long r0 = (long long)blockIdx.y * a.rows;
    const long long r1 = r0 + a.rows < a.total_rows ? r0 + a.rows : a.total_rows;
    const long long p0 = r0 * a.W, p1 = r1 * a.W;   // the strip's pixels [p0, p1) of the batch's B * H * W
    const int H = a.H, W = a.W;

    f32x16 acc[NCI][KS];
#pragma unroll
    for (int j = 0; j < NCI; ++j)
#pragma unroll
        for (int k = 0; k < KS; ++k)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[j][k][e] = 0.f;

    // this half-wave's pixel q = p0 + half, p0 + half + 2, ...: (yq, xq) inside its image, tracked without divisions in the loop
    long long q = p0 + half;
    int xq = (int)(q % W), yq = (int)((q / W) % H);
    const float* gq = a.g + q * a.ldg + co_t * 32 + l;
    const float* xq_p = a.x + q * a.ldx + (cig * NCI) * 32 + l;
    const int dy = ky - PAD;
    const long long row_off = (long long)dy * W * a.ldx;

    // The operands of the NEXT pixel pair are fetched before the MFMAs of the current one are issued.  Every lane always loads: a lane
    // without an operand (tap outside the image, pad pixel, ci tile past the layer's last) reads its channel of pixel 0, which is in
    // bounds, and the value is replaced by 0 when it is USED -- no branch per load, and no wait for a load inside the iteration that
    // issued it.  `m`: bit 0 = the g operand is real, bit 1 + j * KS + kx = that x operand is real.
    auto fetch = [&](float& av, float (&bv)[NCI][KS], unsigned& m) {
        const bool live = q < p1;                   // (false for the pad pixel of an odd strip and for the fetch past the last pair)
        const bool yok = live && (unsigned)(yq + dy) < (unsigned)H;
        av = *(live ? gq : a.g + l);
        m = live ? 1u : 0u;
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
            const bool ok = yok && (unsigned)(xq + kx - PAD) < (unsigned)W;
            const float* px = xq_p + row_off + (long long)(kx - PAD) * a.ldx;
#pragma unroll
            for (int j = 0; j < NCI; ++j) {
                const bool okj = ok && cig * NCI + j < a.nci;
                bv[j][kx] = *(okj ? px + j * 32 : a.x + l);
                m |= okj ? 2u << (j * KS + kx) : 0u;
            }
        }
        q += 2; gq += 2 * a.ldg; xq_p += 2 * a.ldx;
        xq += 2;
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (xq >= W) { xq -= W; yq = yq + 1 == H ? 0 : yq + 1; }
    };
    float av, bv[NCI][KS];
    unsigned mv;
    fetch(av, bv, mv);
    const long long pairs = (p1 - p0 + 1) / 2;
    for (long long it = 0; it < pairs; ++it) {
        float an, bn[NCI][KS];
        unsigned mn;
        fetch(an, bn, mn);
        const float ag = mv & 1u ? av : 0.f;
#pragma unroll
        for (int kx = 0; kx < KS; ++kx)
#pragma unroll
            for (int j = 0; j < NCI; ++j)          // (a ci tile past the layer's last multiplies zeros and is not written back)
                acc[j][kx] = __builtin_amdgcn_mfma_f32_32x32x2f32(ag, mv & (2u << (j * KS + kx)) ? bv[j][kx] : 0.f, acc[j][kx], 0, 0, 0);
        av = an; mv = mn;
#pragma unroll
        for (int j = 0; j < NCI; ++j)
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) bv[j][kx] = bn[j][kx];
    }

    // D[i][j]: i = co (the A rows), j = ci (the B columns); lane: j = l, i = (e & 3) + 8 * (e >> 2) + 4 * half
    const size_t tile = (size_t)a.cg * a.cx;
#pragma unroll
    for (int j = 0; j < NCI; ++j) {
        if (cig * NCI + j >= a.nci) continue;
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
            float* o = a.ws + ((size_t)blockIdx.y * (KS * KS) + ky * KS + kx) * tile + (size_t)(co_t * 32) * a.cx + (cig * NCI + j) * 32 + l;
#pragma unroll
            for (int e = 0; e < 16; ++e) o[(size_t)((e & 3) + 8 * (e >> 2) + 4 * half) * a.cx] = acc[j][kx][e];
        }
    }
}

// dw[co][ci][tap] = the strips' slots added left to right; one thread per real element, consecutive threads = consecutive ci.
// cin_map (may be null: identity): the channel of x that holds input channel ci of dw -- Mconv1_*: the cat buffer's order -> the reference's
__global__ void __launch_bounds__(256) conv_wgrad_combine_kernel(const float* ws, float* dw, int strips, int T, int cout, int cin, int cg, int cx,
                                                                 const int* cin_map)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)T * cout * cin) return;
    const int ci = (int)(i % cin), co = (int)((i / cin) % cout), tap = (int)(i / ((long long)cin * cout));
    const size_t slot = (size_t)T * cg * cx;
    const float* p = ws + ((size_t)tap * cg + co) * cx + (cin_map ? cin_map[ci] : ci);
    float s = p[0];
    for (int k = 1; k < strips; ++k) s = s + p[(size_t)k * slot];
    dw[((size_t)co * cin + ci) * T + tap] = s;
}

// one thread per (pixel of dy, channel of g's cg): without pool the pixel itself, with pool the 2 x 2 window it came from
__global__ void __launch_bounds__(256) conv_bwd_mask_kernel(const float* dy, const float* z, int ldz, float* g, int B, int H, int W, int cout, int cg,
                                                            int relu, int pool)
{
    const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * Ho * Wo * cg) return;
    const int c = (int)(i % cg);
    const long long op = i / cg;
    const int ox = (int)(op % Wo), oy = (int)((op / Wo) % Ho), n = (int)(op / ((long long)Wo * Ho));
    const bool real = c < cout;
    const float d = real ? dy[(((size_t)n * cout + c) * Ho + oy) * Wo + ox] : 0.f;
    if (!pool) {
        const size_t p = ((size_t)n * H + oy) * W + ox;
        float v = d;
        if (real && relu && !(z[p * ldz + c] > 0.f)) v = 0.f;
        g[p * cg + c] = v;
        return;
    }
    float zz[4] = {0.f, 0.f, 0.f, 0.f};
    int best = 0;
    if (real) {
        float am = 0.f;
        for (int k = 0; k < 4; ++k) {
            const size_t p = ((size_t)n * H + 2 * oy + (k >> 1)) * W + 2 * ox + (k & 1);
            zz[k] = z[p * ldz + c];
            const float av = relu ? fmaxf(zz[k], 0.f) : zz[k];
            if (k == 0 || av > am) { am = av; best = k; }      // strictly greater: the first of equal maxima stays
        }
    }
    for (int k = 0; k < 4; ++k) {
        const size_t p = ((size_t)n * H + 2 * oy + (k >> 1)) * W + 2 * ox + (k & 1);
        float v = k == best ? d : 0.f;
        if (real && relu && !(zz[k] > 0.f)) v = 0.f;
        g[p * cg + c] = v;
    }
}

// grid (slots, cg / 32), 256 threads = 8 pixel lanes x 32 channels: float64 sums, the 8 pixel lanes added in lane order through LDS
__global__ void __launch_bounds__(256) conv_bwd_db_kernel(const float* g, int ldg, double* part, long long npix, int cg)
{
    const int l = threadIdx.x & 31, pr = threadIdx.x >> 5, c = blockIdx.y * 32 + l;
    double s = 0.0;
    for (long long p = (long long)blockIdx.x * 8 + pr; p < npix; p += (long long)gridDim.x * 8) s += (double)g[p * ldg + c];
    __shared__ double lds[8][32];
    lds[pr][l] = s;
    __syncthreads();
    if (pr == 0) {
        double t = lds[0][l];
        for (int k = 1; k < 8; ++k) t += lds[k][l];
        part[(size_t)blockIdx.x * cg + c] = t;
    }
}
__global__ void conv_bwd_db_final_kernel(const double* part, float* db, int slots, int cout, int cg)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= cout) return;
    double s = 0.0;
    for (int k = 0; k < slots; ++k) s += part[(size_t)k * cg + c];
    db[c] = (float)s;
}

int db_slots(long long npix) { const long long n = (npix + 7) / 8; return n < PMX_DB_SLOTS ? (int)n : PMX_DB_SLOTS; }

}  // namespace

int conv_bwd_mask_launch(const float* dy, const float* z, int ldz, float* g, int B, int H, int W, int cout, int cg, int relu, int pool, hipStream_t stream)
{
    PMX_CHECK(cg % 32 == 0 && cg >= cout && (z || !(relu || pool)), PMX_ERR_INVALID, "conv_bwd_mask: bad arguments");
    const long long n = (long long)B * (pool ? H / 2 : H) * (pool ? W / 2 : W) * cg;
    hipLaunchKernelGGL(conv_bwd_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, dy, z, ldz, g, B, H, W, cout, cg, relu, pool);
    PMX_HIP(hipGetLastError());
    return PMX_OK;
}

int conv_bwd_db_launch(const float* g, int ldg, double* part, float* db, long long npix, int cout, int cg, hipStream_t stream)
{
    PMX_CHECK(cg % 32 == 0 && cg >= cout && ldg >= cg && npix >= 1, PMX_ERR_INVALID, "conv_bwd_db: bad arguments");
    const int slots = db_slots(npix);
    hipLaunchKernelGGL(conv_bwd_db_kernel, dim3(slots, cg / 32), dim3(256), 0, stream, g, ldg, part, npix, cg);
    PMX_HIP(hipGetLastError());
    hipLaunchKernelGGL(conv_bwd_db_final_kernel, dim3((cout + 63) / 64), dim3(64), 0, stream, (const double*)part, db, slots, cout, cg);
    PMX_HIP(hipGetLastError());
    return PMX_OK;
}

// the strip rules: wgrad_strips.h (plain C, shared with the tests' stand-alone program)
int conv_wgrad_strips(int B, int H, int cg, int cx, int ks, int forced, int* rows) { return pmx_wgrad_strips_cap(B, H, cg, cx, ks, forced, PMX_WGRAD_MAX_STRIPS, 0, rows); }
int conv_wgrad_trunk_strips(int B, int H, int cg, int cx, int forced, int* rows)
{
    return pmx_wgrad_strips_cap(B, H, cg, cx, 3, forced, PMX_WGRAD_TRUNK_MAX_STRIPS, 1, rows);
}

int conv_wgrad_combine_launch(const float* ws, float* dw, int strips, int ks, int cout, int cin, int cg, int cx, const int* cin_map, hipStream_t stream)
{
    const long long n = (long long)ks * ks * cout * cin;
    hipLaunchKernelGGL(conv_wgrad_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ws, dw, strips, ks * ks, cout, cin, cg, cx, cin_map);
    PMX_HIP(hipGetLastError());
    return PMX_OK;
}

int conv_wgrad_launch(const float* g, int ldg, const float* x, int ldx, float* ws, float* dw, int B, int H, int W, int cout, int cg, int cin, int cx,
                      int ks, int strips, int rows, const int* cin_map, hipStream_t stream, int max_strips)
{
    const long long total = (long long)B * H;
    PMX_CHECK(cg % 32 == 0 && cx % 32 == 0 && cg >= cout && cx >= cin && ldg >= cg && ldx >= cx && (ks == 1 || ks == 3 || ks == 7), PMX_ERR_INVALID,
              "conv_wgrad: bad channels / ksize");
    PMX_CHECK(rows >= 1 && strips >= 1 && strips <= max_strips && (long long)(strips - 1) * rows < total && (long long)strips * rows >= total,
              PMX_ERR_INVALID, "conv_wgrad: %d strips of %d rows do not cover %lld rows", strips, rows, total);
    PMX_CHECK((long long)W * ldx * 4 < (1ll << 31), PMX_ERR_INVALID, "conv_wgrad: row of %d x %d floats too long", W, ldx);
    WgradArgs a;
    a.g = g; a.x = x; a.ws = ws; a.H = H; a.W = W; a.cg = cg; a.cx = cx; a.nco = cg / 32; a.nci = cx / 32; a.ldg = ldg; a.ldx = ldx;
    a.n_units = pmx_wgrad_units(cg, cx, ks); a.rows = rows; a.total_rows = total;
    const dim3 grid((a.n_units + 3) / 4, strips);
    if (ks == 7) hipLaunchKernelGGL((conv_wgrad_kernel<7, 1>), grid, dim3(256), 0, stream, a);
    else if (ks == 3) hipLaunchKernelGGL((conv_wgrad_kernel<3, 2>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((conv_wgrad_kernel<1, 4>), grid, dim3(256), 0, stream, a);
    PMX_HIP(hipGetLastError());
    return conv_wgrad_combine_launch(ws, dw, strips, ks, cout, cin, cg, cx, cin_map, stream);
}

// ------------------------------------------------------------------------------------------ head backward (pmx_backward.hip)
// The elementwise steps between the layers of the chain: NHWC in, NHWC out, one thread per (pixel, channel), every sum a float32 add in
// the order include/pose_mi355x.h (pmx_backward_head) documents.
namespace {

// g = u where a > 0, +0.0f elsewhere (a null: no ReLU, g = u)
__global__ void __launch_bounds__(256) bwd_mask_nhwc_kernel(const float* u, int ldu, const float* a, int lda, float* g, int ldg, long long npix, int nch)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix * nch) return;
    const long long p = i / nch;
    const int ch = (int)(i % nch);
    const float v = u[p * ldu + ch];
    g[p * ldg + ch] = !a || a[p * lda + ch] > 0.f ? v : 0.f;
}

// the gradient at a stage's outputs, [pixel][38 PAF, zeros to 64 | 19 heat, zeros to 128]: loss_grad, then + dx of the next stage's Mconv1_L1,
// then + dx of its Mconv1_L2 (d0 / d1: NHWC in cat channel order, ldd floats per pixel; both null for the last stage run)
__global__ void __launch_bounds__(256) bwd_stage_sum_kernel(const float* lg, const float* d0, const float* d1, int ldd, float* g, long long npix)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix * 128) return;
    const long long p = i >> 7;
    const int ch = (int)(i & 127), k = ch & 63, heat = ch >> 6;
    float v = 0.f;
    if (k < (heat ? PMX_N_HEAT : PMX_N_PAF)) {
        v = lg[p * (PMX_N_PAF + PMX_N_HEAT) + (heat ? PMX_N_PAF : 0) + k];
        if (d0) {
            const int cc = (heat ? PMX_CAT_HEAT : PMX_CAT_PAF) + k;
            v = v + d0[p * ldd + cc];
            v = v + d1[p * ldd + cc];
        }
    }
    g[i] = v;
}

// the gradient at the feature map, [pixel][128]: first ? a + b : (fg + a) + b
__global__ void __launch_bounds__(256) bwd_feat_sum_kernel(float* fg, const float* a, const float* b, int ld, int first, long long npix)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix * 128) return;
    const long long p = i >> 7;
    const int ch = (int)(i & 127);
    const float va = a[p * ld + ch], vb = b[p * ld + ch];
    fg[i] = first ? va + vb : (fg[i] + va) + vb;
}

__global__ void __launch_bounds__(256) bwd_copy_cols_kernel(const float* src, int lds, float* dst, int ldd, long long npix, int nch)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix * nch) return;
    const long long p = i / nch;
    const int ch = (int)(i % nch);
    dst[p * ldd + ch] = src[p * lds + ch];
}

unsigned bwd_blocks(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

int bwd_mask_nhwc_launch(const float* u, int ldu, const float* a, int lda, float* g, int ldg, long long npix, int nch, hipStream_t stream)
{
    PMX_CHECK(u && g && npix >= 1 && nch >= 1 && ldu >= nch && ldg >= nch && (!a || lda >= nch), PMX_ERR_INVALID, "bwd_mask_nhwc: bad arguments");
    hipLaunchKernelGGL(bwd_mask_nhwc_kernel, dim3(bwd_blocks(npix * nch)), dim3(256), 0, stream, u, ldu, a, lda, g, ldg, npix, nch);
    PMX_HIP(hipGetLastError());
    return PMX_OK;
}

int bwd_stage_sum_launch(const float* lg, const float* d0, const float* d1, int ldd, float* g, long long npix, hipStream_t stream)
{
    PMX_CHECK(lg && g && npix >= 1 && !d0 == !d1 && (!d0 || ldd >= PMX_CAT_C), PMX_ERR_INVALID, "bwd_stage_sum: bad arguments");
    hipLaunchKernelGGL(bwd_stage_sum_kernel, dim3(bwd_blocks(npix * 128)), dim3(256), 0, stream, lg, d0, d1, ldd, g, npix);
    PMX_HIP(hipGetLastError());
    return PMX_OK;
}

int bwd_feat_sum_launch(float* fg, const float* a, const float* b, int ld, int first, long long npix, hipStream_t stream)
{
    PMX_CHECK(fg && a && b && npix >= 1 && ld >= 128, PMX_ERR_INVALID, "bwd_feat_sum: bad arguments");
    hipLaunchKernelGGL(bwd_feat_sum_kernel, dim3(bwd_blocks(npix * 128)), dim3(256), 0, stream, fg, a, b, ld, first, npix);
    PMX_HIP(hipGetLastError());
    return PMX_OK;
}

int bwd_copy_cols_launch(const float* src, int lds, float* dst, int ldd, long long npix, int nch, hipStream_t stream)
{
    PMX_CHECK(src && dst && npix >= 1 && nch >= 1 && lds >= nch && ldd >= nch, PMX_ERR_INVALID, "bwd_copy_cols: bad arguments");
    hipLaunchKernelGGL(bwd_copy_cols_kernel, dim3(bwd_blocks(npix * nch)), dim3(256), 0, stream, src, lds, dst, ldd, npix, nch);
    PMX_HIP(hipGetLastError());
    return PMX_OK;
}

// ------------------------------------------------------------------------------------------ trunk backward (pmx_backward.hip)
// conv1_1's weight gradient, dw[64][3][3][3]: x is the network input at PMX_IN_C = 16 floats per pixel, 3 of them real, so the generic
// kernel's 32-channel x tiles would be 29 / 32 zeros.  Here the 32 B columns of the MFMA are the 27 (ci, tap) pairs themselves, column
// l = ci * 9 + ky * 3 + kx -- the OIHW order of one co's 27 weights -- and 5 zero columns: lane l < 27 loads x[p + tap(l)][ci(l)], zero
// outside the image.  A = 32 co of pixel p (lanes 0-31) and of pixel p + 1 (lanes 32-63), as in conv_wgrad_kernel.  One wave owns one strip
// and keeps BOTH co tiles (2 x 16 accumulator registers), so x is fetched once per pixel pair: per pair a lane loads one float of x and
// two of g.  The four waves of a block are four consecutive strips.  A strip's accumulators go to its slot [strip][co 64][32] of the
// workspace; conv1_wgrad_combine_kernel adds the slots left to right.  The order per element is conv_wgrad_kernel's (the header's twin
// with cin = 3): fmaf(g, x, acc) over the strip's pixels in row-major order, pixel p before p + 1 inside an MFMA.  No atomics.
namespace {

struct Wgrad1Args {
    const float* g; const float* x; float* ws;
    int H, W, rows, strips, ldg;                    // rows: image rows per strip; ldg: floats per pixel of g (>= 64)
    long long total_rows;                           // B * H
};

__global__ void __launch_bounds__(256) conv1_wgrad_kernel(Wgrad1Args a)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5, l = lane & 31;
    const int strip = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
    if (strip >= a.strips) return;                  // (no barrier below: a wave may leave alone)
    const long long r0 = (long long)strip * a.rows;
    const long long r1 = r0 + a.rows < a.total_rows ? r0 + a.rows : a.total_rows;
    const long long p0 = r0 * a.W, p1 = r1 * a.W;   // the strip's pixels [p0, p1) of the batch's B * H * W
    const int H = a.H, W = a.W;
    const bool col = l < 27;                        // (columns 27 .. 31 multiply zeros and are not written back)
    const int ci = col ? l / 9 : 0, tap = col ? l % 9 : 4, dy = tap / 3 - 1, dx = tap % 3 - 1;

    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

    long long q = p0 + half;
    int xq = (int)(q % W), yq = (int)((q / W) % H);
    const float* gq = a.g + q * a.ldg + l;
    const float* xp = a.x + (q + (long long)dy * W + dx) * PMX_IN_C + ci;
    // as in conv_wgrad_kernel: the operands of the NEXT pixel pair are fetched before the MFMAs of the current one; every lane always
    // loads -- a lane without an operand reads an address that is in bounds -- and the value is replaced by 0 when it is used
    auto fetch = [&](float& g0, float& g1, float& xv, unsigned& m) {
        const bool live = q < p1;
        const bool ok = live && col && (unsigned)(yq + dy) < (unsigned)H && (unsigned)(xq + dx) < (unsigned)W;
        const float* gp = live ? gq : a.g + l;
        g0 = gp[0]; g1 = gp[32];
        xv = *(ok ? xp : a.x + (l & 15));
        m = (live ? 1u : 0u) | (ok ? 2u : 0u);
        q += 2; gq += 2 * a.ldg; xp += 2 * PMX_IN_C;
        xq += 2;
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (xq >= W) { xq -= W; yq = yq + 1 == H ? 0 : yq + 1; }
    };
    float g0, g1, xv;
    unsigned mv;
    fetch(g0, g1, xv, mv);
    const long long pairs = (p1 - p0 + 1) / 2;
    for (long long it = 0; it < pairs; ++it) {
        float n0, n1, nx;
        unsigned mn;
        fetch(n0, n1, nx, mn);
        const float b = mv & 2u ? xv : 0.f;
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(mv & 1u ? g0 : 0.f, b, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(mv & 1u ? g1 : 0.f, b, acc[1], 0, 0, 0);
        g0 = n0; g1 = n1; xv = nx; mv = mn;
    }
    // D[i][j]: i = co (the A rows), j = column l; lane: j = l, i = (e & 3) + 8 * (e >> 2) + 4 * half
    if (!col) return;
    float* o = a.ws + (size_t)strip * (64 * 32) + l;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[(size_t)(t * 32 + (e & 3) + 8 * (e >> 2) + 4 * half) * 32] = acc[t][e];
}

// dw[co][ci][ky][kx] = dw[co * 27 + l]: the strips' slots added left to right; one thread per element
__global__ void __launch_bounds__(64) conv1_wgrad_combine_kernel(const float* ws, float* dw, int strips)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= 64 * 27) return;
    const float* p = ws + (size_t)(i / 27) * 32 + i % 27;
    float s = p[0];
    for (int k = 1; k < strips; ++k) s = s + p[(size_t)k * (64 * 32)];
    dw[i] = s;
}

// F.max_pooling_2d(a, 2, 2) on NHWC, one thread per (pooled pixel, channel): the first maximum in window order (0,0), (0,1), (1,0), (1,1)
__global__ void __launch_bounds__(256) maxpool_nhwc_kernel(const float* a, int lda, float* out, int ldo, int B, int H, int W, int nch)
{
    const int Ho = H / 2, Wo = W / 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * Ho * Wo * nch) return;
    const int ch = (int)(i % nch);
    const long long op = i / nch;
    const int ox = (int)(op % Wo), oy = (int)((op / Wo) % Ho), n = (int)(op / ((long long)Wo * Ho));
    const float* p = a + (((size_t)n * H + 2 * oy) * W + 2 * ox) * lda + ch;
    float m = p[0];
    const float v1 = p[lda], v2 = p[(size_t)W * lda], v3 = p[(size_t)(W + 1) * lda];
    if (v1 > m) m = v1;
    if (v2 > m) m = v2;
    if (v3 > m) m = v3;
    out[(size_t)op * ldo + ch] = m;
}

// the gradient through relu + 2 x 2 max-pool, read from the post-ReLU, pre-pool output a alone: u (pooled size) goes to the FIRST maximum of
// its window of a (strictly greater in window order, conv_bwd_mask_kernel's rule) if that a > 0; +0.0f in the other positions.  One thread
// per (pooled pixel, channel) writes the four elements of its window: every element of g by exactly one thread.
__global__ void __launch_bounds__(256) pool_bwd_nhwc_kernel(const float* u, int ldu, const float* a, int lda, float* g, int ldg, int B, int H, int W, int nch)
{
    const int Ho = H / 2, Wo = W / 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * Ho * Wo * nch) return;
    const int ch = (int)(i % nch);
    const long long op = i / nch;
    const int ox = (int)(op % Wo), oy = (int)((op / Wo) % Ho), n = (int)(op / ((long long)Wo * Ho));
    const size_t base = ((size_t)n * H + 2 * oy) * W + 2 * ox;
    float av[4], am = 0.f;
    int best = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        av[k] = a[(base + (size_t)(k >> 1) * W + (k & 1)) * lda + ch];
        if (k == 0 || av[k] > am) { am = av[k]; best = k; }      // strictly greater: the first of equal maxima stays
    }
    const float d = u[(size_t)op * ldu + ch];
#pragma unroll
    for (int k = 0; k < 4; ++k) g[(base + (size_t)(k >> 1) * W + (k & 1)) * ldg + ch] = k == best && av[k] > 0.f ? d : 0.f;
}

// The range census of a g slice (pmx_backward_g_census): where the f16 kernels' conversion r = f16_rn_sat(v) puts the nch channels of every
// pixel.  counts[0] v != 0, [1] v != 0 and r == 0, [2] r an f16 subnormal, [3] |v| > 65504, [4] NaN.  Every thread counts its elements of a
// grid-stride loop, the block adds its threads' counts in LDS, and thread t < 5 adds the block's count t to counts[t] with one INTEGER atomic:
// integer sums do not depend on the order, so the result is the same on every run.
__global__ void __launch_bounds__(256) bwd_g_census_kernel(const float* g, int ldg, long long npix, int nch, unsigned long long* counts)
{
    unsigned n[5] = {0u, 0u, 0u, 0u, 0u};
    const long long total = npix * nch, stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const long long pix = i / nch;
        const float v = g[(size_t)pix * ldg + (int)(i - pix * nch)];
        const unsigned mag = f16_rn_sat(v) & 0x7fffu;
        n[0] += v != 0.f ? 1u : 0u;
        n[1] += v != 0.f && mag == 0u ? 1u : 0u;
        n[2] += mag > 0u && mag < 0x0400u ? 1u : 0u;
        n[3] += fabsf(v) > 65504.f ? 1u : 0u;
        n[4] += v != v ? 1u : 0u;
    }
    __shared__ unsigned long long lds[5][256];
#pragma unroll
    for (int k = 0; k < 5; ++k) lds[k][threadIdx.x] = n[k];
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w)
#pragma unroll
            for (int k = 0; k < 5; ++k) lds[k][threadIdx.x] += lds[k][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < 5 && lds[threadIdx.x][0]) atomicAdd(&counts[threadIdx.x], lds[threadIdx.x][0]);
}

}  // namespace

int bwd_g_census_launch(const float* g, int ldg, long long npix, int nch, unsigned long long* counts, hipStream_t stream)
{
    PMX_CHECK(g && counts && npix >= 1 && nch >= 1 && ldg >= nch, PMX_ERR_INVALID, "g census: bad arguments");
    const unsigned blocks = npix * nch < 1024ll * 256 ? bwd_blocks(npix * nch) : 1024u;
    hipLaunchKernelGGL(bwd_g_census_kernel, dim3(blocks), dim3(256), 0, stream, g, ldg, npix, nch, counts);
    PMX_HIP(hipGetLastError());
    return PMX_OK;
}

int conv1_wgrad_strips(int B, int H, int forced, int* rows) { return pmx_wgrad_conv1_strips(B, H, forced, PMX_WGRAD_CONV1_STRIPS, rows); }

int conv1_wgrad_launch(const float* g, int ldg, const float* x16, float* ws, float* dw, int B, int H, int W, int strips, int rows, hipStream_t stream)
{
    const long long total = (long long)B * H;
    PMX_CHECK(g && x16 && ws && dw && B >= 1 && H >= 1 && W >= 1 && ldg >= 64, PMX_ERR_INVALID, "conv1_wgrad: bad arguments");
    PMX_CHECK(rows >= 1 && strips >= 1 && strips < 2 * PMX_WGRAD_CONV1_STRIPS && (long long)(strips - 1) * rows < total && (long long)strips * rows >= total,
              PMX_ERR_INVALID, "conv1_wgrad: %d strips of %d rows do not cover %lld rows", strips, rows, total);
    PMX_CHECK(total * W >= 2, PMX_ERR_INVALID, "conv1_wgrad: %lld pixels", total * W);      // (a lane without an operand reads floats 0 .. 31 of g, 0 .. 15 of x)
    Wgrad1Args a;
    a.g = g; a.x = x16; a.ws = ws; a.H = H; a.W = W; a.rows = rows; a.strips = strips; a.ldg = ldg; a.total_rows = total;
    hipLaunchKernelGGL(conv1_wgrad_kernel, dim3((strips + 3) / 4), dim3(256), 0, stream, a);
    PMX_HIP(hipGetLastError());
    hipLaunchKernelGGL(conv1_wgrad_combine_kernel, dim3(27), dim3(64), 0, stream, (const float*)ws, dw, strips);
    PMX_HIP(hipGetLastError());
    return PMX_OK;
}

int maxpool_nhwc_launch(const float* a, int lda, float* out, int ldo, int B, int H, int W, int nch, hipStream_t stream)
{
    PMX_CHECK(a && out && B >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && nch >= 1 && lda >= nch && ldo >= nch, PMX_ERR_INVALID,
              "maxpool_nhwc: bad arguments");
    hipLaunchKernelGGL(maxpool_nhwc_kernel, dim3(bwd_blocks((long long)B * (H / 2) * (W / 2) * nch)), dim3(256), 0, stream, a, lda, out, ldo, B, H, W, nch);
    PMX_HIP(hipGetLastError());
    return PMX_OK;
}

int pool_bwd_nhwc_launch(const float* u, int ldu, const float* a, int lda, float* g, int ldg, int B, int H, int W, int nch, hipStream_t stream)
{
    PMX_CHECK(u && a && g && B >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && nch >= 1 && ldu >= nch && lda >= nch && ldg >= nch,
              PMX_ERR_INVALID, "pool_bwd_nhwc: bad arguments");
    hipLaunchKernelGGL(pool_bwd_nhwc_kernel, dim3(bwd_blocks((long long)B * (H / 2) * (W / 2) * nch)), dim3(256), 0, stream, u, ldu, a, lda, g, ldg, B, H, W, nch);
    PMX_HIP(hipGetLastError());
    return PMX_OK;
}
