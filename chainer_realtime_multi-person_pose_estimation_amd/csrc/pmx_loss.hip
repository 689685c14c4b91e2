// pmx_loss.hip -- validation loss on the device: Validator.evaluate (train_coco_pose_estimation.py:129-159) without the data loader.
//
//   label kernels   generate_heatmaps + generate_pafs (coco_data_loader.py:208-268) evaluated from the poses in float64, product by product
//                   as NumPy does (this file is compiled with -ffp-contract=off), cast to float32.  Form (a): every pixel of one image
//                   (pmx_get_labels).  Form (b): only the four corner pixels each map pixel of h/8 x w/8 needs, combined as F.resize_images
//                   does (:57-60; oracle/postprocess_ref.py::resize_images_ref) and written as targets [image][map pixel][38 PAF | 19 heat];
//                   the same pass resizes the ignore mask.  The batch x 57 x h x w label maps never exist.
//   loss kernel     one launch per stage, enqueued by the forward right after the stage's last launch (pmx_api.hip): per branch the float64
//                   sum of ((double)d * d), d = y - t in float32, ignored pixels skipped; wave-64 shuffle reduction, LDS across the four
//                   waves, one partial per block and branch in a fixed slot.  A last launch adds the partials in slot order and divides by
//                   the element counts.  No atomics, a fixed grid per problem size: the same bits on every run.
// Nothing here synchronises or copies to the host between the stages; only the getters do.
#include "pmx_ctx.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#pragma clang fp contract(off)

namespace {

constexpr int N_CH = PMX_N_PAF + PMX_N_HEAT;            // 57 target channels per map pixel
constexpr int POSE_D = PMX_N_JOINTS * 3;                // doubles per person

__constant__ int LIMB_FROM[PMX_N_LIMBS] = {1, 8, 9, 1, 11, 12, 1, 2, 3, 2, 1, 5, 6, 5, 1, 0, 0, 14, 15};
__constant__ int LIMB_TO[PMX_N_LIMBS] = {8, 9, 10, 11, 12, 13, 2, 3, 4, 16, 5, 6, 7, 17, 0, 14, 15, 16, 17};

// the corner-aligned grid (h, w) -> (h/8, w/8): per map column / row the two source indices and their float64 weights
struct LossGrid { const double *xlo, *xhi, *ylo, *yhi; const int *xi0, *xi1, *yi0, *yi1; };

// generate_heatmaps (:216-229) for joint type j at pixel (x, y): max over the people with v > 0 of exp(-0.5 * d2 / sigma**2), from 0
__device__ double heat_joint(const double* P, int n, int j, double x, double y, double s2)
{
    double m = 0.0;
    for (int p = 0; p < n; ++p) {
        const double* q = P + (size_t)p * POSE_D + j * 3;
        if (!(q[2] > 0)) continue;
        const double dx = x - q[0], dy = y - q[1];
        const double d2 = dx * dx + dy * dy;
        const double g = exp(-0.5 * d2 / s2);
        if (g > m) m = g;
    }
    return m;
}
__device__ double heat_background(const double* P, int n, double x, double y, double s2)     // :225-227
{
    double m = 0.0;
    for (int j = 0; j < PMX_N_JOINTS; ++j) {
        const double g = heat_joint(P, n, j, x, y, s2);
        if (g > m) m = g;
    }
    return 1 - m;
}
// generate_pafs (:251-268) / generate_constant_paf (:232-249) for limb `limb` at pixel (x, y)
__device__ void paf_limb(const double* P, int n, int limb, double x, double y, double width, double& ox, double& oy)
{
    const double c = 6.123233995736766e-17, s = 1.0;      // np.cos(np.pi / 2), np.sin(np.pi / 2)
    const int ja = LIMB_FROM[limb], jb = LIMB_TO[limb];
    double ax = 0.0, ay = 0.0, cnt = 0.0;
    for (int p = 0; p < n; ++p) {
        const double* a = P + (size_t)p * POSE_D + ja * 3;
        const double* b = P + (size_t)p * POSE_D + jb * 3;
        if (!(a[2] > 0 && b[2] > 0)) continue;                 // :260
        if (a[0] == b[0] && a[1] == b[1]) continue;            // :233
        const double dx = b[0] - a[0], dy = b[1] - a[1];
        const double dist = sqrt(dx * dx + dy * dy);
        const double ux = dx / dist, uy = dy / dist;
        const double vx = c * ux + s * uy, vy = -s * ux + c * uy;      // np.dot(rot_matrix, unit_vector)
        const double gx = x - a[0], gy = y - a[1];
        const double hor = ux * gx + uy * gy;
        const double ver = vx * gx + vy * gy;
        if (!(0 <= hor && hor <= dist && fabs(ver) <= width)) continue;
        if (ux != 0 || uy != 0) cnt += 1;                      // :262-263
        ax += ux; ay += uy;
    }
    if (cnt > 0) { ax /= cnt; ay /= cnt; }                     // :266
    ox = ax; oy = ay;
}

// F.resize_images' four-term sum: float32 products, added left to right
__device__ inline float combine4(float w1, float w2, float w3, float w4, float x00, float x01, float x10, float x11)
{
    return w1 * x00 + w2 * x01 + w3 * x10 + w4 * x11;
}

struct Corner { int x0, x1, y0, y1; float w1, w2, w3, w4; };
__device__ inline Corner corner_of(const LossGrid& g, int ox, int oy)
{
    Corner k;
    k.x0 = g.xi0[ox]; k.x1 = g.xi1[ox]; k.y0 = g.yi0[oy]; k.y1 = g.yi1[oy];
    k.w1 = (float)(g.ylo[oy] * g.xlo[ox]); k.w2 = (float)(g.ylo[oy] * g.xhi[ox]);
    k.w3 = (float)(g.yhi[oy] * g.xlo[ox]); k.w4 = (float)(g.yhi[oy] * g.xhi[ox]);
    return k;
}
__device__ inline uint8_t mask_at(const uint8_t* mask_in, const Corner& k, size_t img_off, int w)
{
    if (!mask_in) return 0;
    const uint8_t* m = mask_in + img_off;
    const float s = combine4(k.w1, k.w2, k.w3, k.w4, m[(size_t)k.y0 * w + k.x0] ? 1.f : 0.f, m[(size_t)k.y0 * w + k.x1] ? 1.f : 0.f,
                             m[(size_t)k.y1 * w + k.x0] ? 1.f : 0.f, m[(size_t)k.y1 * w + k.x1] ? 1.f : 0.f);
    return s > 0 ? 1 : 0;
}

// form (b).  grid (map pixels / 256, 39 tasks, images): tasks 0..18 = limbs (two channels), 19..36 = joint types, 37 = background, 38 = mask
__global__ void __launch_bounds__(256) loss_targets_kernel(const double* poses, const int* off, LossGrid g, const uint8_t* mask_in, float* tgt,
                                                           uint8_t* mask, int h, int w, int fh, int fw, double s2, double width)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= fh * fw) return;
    const int task = blockIdx.y, b = blockIdx.z;
    const Corner k = corner_of(g, p % fw, p / fw);
    const double* P = poses + (size_t)off[b] * POSE_D;
    const int n = off[b + 1] - off[b];
    const size_t pix = (size_t)b * fh * fw + p;
    float* t = tgt + pix * N_CH;
    const double xs[2] = {(double)k.x0, (double)k.x1}, ys[2] = {(double)k.y0, (double)k.y1};
    if (task < PMX_N_LIMBS) {
        float vx[4], vy[4];
        for (int i = 0; i < 4; ++i) {
            double ox, oy;
            paf_limb(P, n, task, xs[i & 1], ys[i >> 1], width, ox, oy);
            vx[i] = (float)ox; vy[i] = (float)oy;
        }
        t[2 * task] = combine4(k.w1, k.w2, k.w3, k.w4, vx[0], vx[1], vx[2], vx[3]);
        t[2 * task + 1] = combine4(k.w1, k.w2, k.w3, k.w4, vy[0], vy[1], vy[2], vy[3]);
    } else if (task < PMX_N_LIMBS + PMX_N_HEAT) {
        const int j = task - PMX_N_LIMBS;
        float v[4];
        for (int i = 0; i < 4; ++i)
            v[i] = (float)(j < PMX_N_JOINTS ? heat_joint(P, n, j, xs[i & 1], ys[i >> 1], s2) : heat_background(P, n, xs[i & 1], ys[i >> 1], s2));
        t[PMX_N_PAF + j] = combine4(k.w1, k.w2, k.w3, k.w4, v[0], v[1], v[2], v[3]);
    } else {
        mask[pix] = mask_at(mask_in, k, (size_t)b * h * w, w);
    }
}

// form (a).  grid (pixels / 256, 38 tasks): planar out[57][h * w] of one image
__global__ void __launch_bounds__(256) loss_labels_kernel(const double* P, int n, float* out, int h, int w, double s2, double width)
{
    const long long hw = (long long)h * w;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const int task = blockIdx.y;
    const double x = (double)(p % w), y = (double)(p / w);
    if (task < PMX_N_LIMBS) {
        double ox, oy;
        paf_limb(P, n, task, x, y, width, ox, oy);
        out[(long long)(2 * task) * hw + p] = (float)ox;
        out[(long long)(2 * task + 1) * hw + p] = (float)oy;
    } else {
        const int j = task - PMX_N_LIMBS;
        out[(long long)(PMX_N_PAF + j) * hw + p] = (float)(j < PMX_N_JOINTS ? heat_joint(P, n, j, x, y, s2) : heat_background(P, n, x, y, s2));
    }
}

// caller-made full-resolution maps of ONE image (planar full[57][h * w]) -> its targets.  grid (map pixels / 256, 58): channel 57 = the mask
__global__ void __launch_bounds__(256) loss_resize_kernel(const float* full, LossGrid g, const uint8_t* mask_in, float* tgt, uint8_t* mask, int b,
                                                          int h, int w, int fh, int fw)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= fh * fw) return;
    const int ch = blockIdx.y;
    const Corner k = corner_of(g, p % fw, p / fw);
    const size_t pix = (size_t)b * fh * fw + p;
    if (ch < N_CH) {
        const float* s = full + (size_t)ch * h * w;
        tgt[pix * N_CH + ch] = combine4(k.w1, k.w2, k.w3, k.w4, s[(size_t)k.y0 * w + k.x0], s[(size_t)k.y0 * w + k.x1],
                                        s[(size_t)k.y1 * w + k.x0], s[(size_t)k.y1 * w + k.x1]);
    } else {
        mask[pix] = mask_at(mask_in, k, (size_t)b * h * w, w);
    }
}

// where a stage's outputs live: element (image b, channel ch, map pixel p) of the PAF = paf[b * sb_p + p * sp + ch * sc]
struct LossSrc { const float* paf; const float* heat; long long sb_p, sb_h, sp, sc; };

__global__ void __launch_bounds__(256) loss_stage_kernel(LossSrc y, const float* tgt, const uint8_t* mask, double* part, long long npix, int fhw)
{
    double sum_p = 0.0, sum_h = 0.0;
    const long long total = npix * N_CH, stride = (long long)gridDim.x * 256;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const long long pix = e / N_CH;
        if (mask[pix]) continue;                               // :62-63: target := output, the difference is 0
        const int ch = (int)(e - pix * N_CH);
        const long long b = pix / fhw, p = pix - b * fhw;
        const float yv = ch < PMX_N_PAF ? y.paf[b * y.sb_p + p * y.sp + ch * y.sc] : y.heat[b * y.sb_h + p * y.sp + (ch - PMX_N_PAF) * y.sc];
        const float d = yv - tgt[e];
        const double dd = (double)d * (double)d;
        if (ch < PMX_N_PAF) sum_p += dd; else sum_h += dd;
    }
    for (int o = 32; o > 0; o >>= 1) {
        sum_p += __shfl_down(sum_p, o);
        sum_h += __shfl_down(sum_h, o);
    }
    __shared__ double lds[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { lds[0][wave] = sum_p; lds[1][wave] = sum_h; }
    __syncthreads();
    if (threadIdx.x < 2) part[blockIdx.x * 2 + threadIdx.x] = ((lds[threadIdx.x][0] + lds[threadIdx.x][1]) + lds[threadIdx.x][2]) + lds[threadIdx.x][3];
}

// d(total_loss)/dy of one stage (pmx_loss_grad_enable): F.mean_squared_error's backward with gy = 1, one thread per element of
// grad[image][map pixel][38 | 19]: c * (y - t) as ONE float32 product, +0.0f where the resized mask is set
__global__ void __launch_bounds__(256) loss_grad_kernel(LossSrc y, const float* tgt, const uint8_t* mask, float* grad, long long npix, int fhw,
                                                        float c_paf, float c_heat)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= npix * N_CH) return;
    const long long pix = e / N_CH;
    float gv = 0.0f;
    if (!mask[pix]) {
        const int ch = (int)(e - pix * N_CH);
        const long long b = pix / fhw, p = pix - b * fhw;
        const float yv = ch < PMX_N_PAF ? y.paf[b * y.sb_p + p * y.sp + ch * y.sc] : y.heat[b * y.sb_h + p * y.sp + (ch - PMX_N_PAF) * y.sc];
        const float d = yv - tgt[e];
        gv = (ch < PMX_N_PAF ? c_paf : c_heat) * d;
    }
    grad[e] = gv;
}

// out[slot][branch] for the slots [slot0, slot1): the partials of the first `nb` blocks added in block order, / elements; slots >= valid: 0
__global__ void loss_final_kernel(const double* part, double* out, int slot0, int slot1, int valid, int nb, double n_paf, double n_heat)
{
    const int t = threadIdx.x;
    if (t >= 2 * (slot1 - slot0)) return;
    const int slot = slot0 + t / 2, br = t % 2;
    double s = 0.0;
    if (slot < valid) {
        const double* q = part + (size_t)slot * PMX_LOSS_MAX_BLOCKS * 2 + br;
        for (int i = 0; i < nb; ++i) s += q[2 * i];
        s /= br ? n_heat : n_paf;
    }
    out[slot * 2 + br] = s;
}

LossGrid grid_view(const pmx_ctx* c)
{
    const PPTables& t = c->ls_tab;
    return LossGrid{t.xlo, t.xhi, t.ylo, t.yhi, t.xi0, t.xi1, t.yi0, t.yi1};
}

// the grid block (pp_tables.h) of (h, w) -> (h/8, w/8) on the device (uploaded when the size changes: a setup step, synchronises then)
int ensure_grid(pmx_ctx* c, int h, int w)
{
    if (c->ls_grid_h == h && c->ls_grid_w == w) return PMX_OK;
    const int fh = h / 8, fw = w / 8;
    const size_t bytes = pp_grid_bytes(fh, fw);
    c->ls_grid_h = 0;
    PMX_HIP(hipStreamSynchronize(c->stream));          // a queued label launch may still read the old grid
    if (bytes > c->ls_grid.capacity()) if (int rc = c->ls_grid.alloc(bytes)) return rc;
    std::vector<double> host(bytes / sizeof(double));
    pp_grid_build(h, w, fh, fw, 0, host.data(), c->ls_grid.get(), c->ls_tab);
    PMX_HIP(hipMemcpy(c->ls_grid, host.data(), bytes, hipMemcpyHostToDevice));
    c->ls_grid_h = h; c->ls_grid_w = w;
    return PMX_OK;
}

// the buffers every target set needs, at the context's capacity, allocated by the first use of the feature
int ensure_target_buffers(pmx_ctx* c)
{
    const size_t npix = (size_t)c->max_batch * ((size_t)c->max_h * c->max_w / 64);
    int rc;
    if ((rc = c->ls_tgt.ensure(npix * N_CH, c->stream)) || (rc = c->ls_mask.ensure(npix, c->stream))) return rc;
    if ((rc = c->ls_part.ensure((size_t)PMX_LOSS_SLOTS * PMX_LOSS_MAX_BLOCKS * 2, c->stream))) return rc;
    return c->ls_out.ensure(2 * PMX_LOSS_SLOTS, c->stream);
}

int check_common(pmx_ctx* c, const char* what, int batch, int h, int w)
{
    PMX_CHECK(batch >= 1 && batch <= c->max_batch, PMX_ERR_CAPACITY, "%s: batch %d outside 1..%d", what, batch, c->max_batch);
    PMX_CHECK(h >= 8 && w >= 8 && h % 8 == 0 && w % 8 == 0, PMX_ERR_INVALID, "%s: h, w must be multiples of 8 (got %d x %d)", what, h, w);
    PMX_CHECK((size_t)h * w <= (size_t)c->max_h * c->max_w, PMX_ERR_CAPACITY, "%s: %d x %d exceeds the context capacity %d x %d", what, h, w,
              c->max_h, c->max_w);
    return PMX_OK;
}
#define LOSS_POSENET(c, what) \
    PMX_CHECK((c)->kind == NET_POSE, PMX_ERR_STATE, what ": posenet contexts only (the loss is that of CocoPoseNet's six stages)")

int blocks_for(long long threads) { return (int)((threads + 255) / 256); }

// the loss launch of one slot over `src`
int launch_stage(pmx_ctx* c, const char* label, int slot, const LossSrc& src, int B, int fh, int fw)
{
    const long long npix = (long long)B * fh * fw;
    long long nb = (npix * N_CH + 255) / 256;
    if (nb > PMX_LOSS_MAX_BLOCKS) nb = PMX_LOSS_MAX_BLOCKS;
    int rc;
    if ((rc = pmx_prof_begin(c, label, (double)npix * (2 * N_CH * 4 + 1)))) return rc;
    hipLaunchKernelGGL(loss_stage_kernel, dim3((unsigned)nb), dim3(256), 0, c->stream, src, (const float*)c->ls_tgt, (const uint8_t*)c->ls_mask,
                       c->ls_part + (size_t)slot * PMX_LOSS_MAX_BLOCKS * 2, npix, fh * fw);
    PMX_HIP(hipGetLastError());
    return pmx_prof_end(c);
}
int launch_final(pmx_ctx* c, int slot0, int slot1, int valid, int B, int fh, int fw)
{
    const long long npix = (long long)B * fh * fw;
    long long nb = (npix * N_CH + 255) / 256;
    if (nb > PMX_LOSS_MAX_BLOCKS) nb = PMX_LOSS_MAX_BLOCKS;
    int rc;
    if ((rc = pmx_prof_begin(c, "loss_final|pmx_loss_final", 0))) return rc;
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(64), 0, c->stream, (const double*)c->ls_part, (double*)c->ls_out, slot0, slot1, valid, (int)nb,
                       (double)npix * PMX_N_PAF, (double)npix * PMX_N_HEAT);
    PMX_HIP(hipGetLastError());
    return pmx_prof_end(c);
}

}  // namespace

// ------------------------------------------------------------------------------------------ the forward's hook
int pmx_loss_check(pmx_ctx* c, int B, int H, int W)
{
    PMX_CHECK(c->ls_B > 0, PMX_ERR_STATE, "forward with the validation-loss hook on: no targets (call pmx_loss_set_poses / pmx_loss_set_targets first)");
    PMX_CHECK(c->ls_B == B && c->ls_h == H && c->ls_w == W, PMX_ERR_STATE,
              "forward with the validation-loss hook on: the targets are those of %d x %d x %d, the batch is %d x %d x %d", c->ls_B, c->ls_h,
              c->ls_w, B, H, W);
    return PMX_OK;
}

int pmx_loss_stage(pmx_ctx* c, int stage, int B, int fh, int fw)
{
    PMX_CHECK(stage >= 1 && stage < PMX_LOSS_SLOTS && c->ls_B == B && c->ls_h == fh * 8 && c->ls_w == fw * 8, PMX_ERR_STATE,
              "pmx_loss_stage: stage %d of a %d x %d x %d forward against targets of %d x %d x %d", stage, B, fh * 8, fw * 8, c->ls_B, c->ls_h, c->ls_w);
    char label[48];
    snprintf(label, sizeof label, "loss_stage%d|pmx_loss", stage);
    const long long fhw = (long long)fh * fw;
    const LossSrc src = {c->cat + PMX_CAT_PAF, c->cat + PMX_CAT_HEAT, fhw * PMX_CAT_C, fhw * PMX_CAT_C, PMX_CAT_C, 1};
    if (int rc = launch_stage(c, label, stage - 1, src, B, fh, fw)) return rc;
    if (!c->lg_on) return PMX_OK;
    // the stage's gradient, a launch of its own
    const long long npix = (long long)B * fhw;
    PMX_CHECK(c->ls_grad.capacity() >= (size_t)(PMX_LOSS_SLOTS - 1) * npix * N_CH, PMX_ERR_STATE, "pmx_loss_stage: no gradient buffer");
    if (stage == 1) c->lg_stages = 0;                       // until pmx_loss_finish: the buffer is being rewritten
    // option "loss_scale_log2" = k: both constants times 2^k, on the host and exact (ldexpf of a normal float32 far from the range's ends);
    // the kernel's one product c * d then carries the factor, and everything downstream is linear
    const int k = c->opt_loss_scale_log2;
    snprintf(label, sizeof label, "loss_grad%d|pmx_loss_grad", stage);
    int rc;
    if ((rc = pmx_prof_begin(c, label, (double)npix * (3 * N_CH * 4 + 1)))) return rc;
    hipLaunchKernelGGL(loss_grad_kernel, dim3(blocks_for(npix * N_CH)), dim3(256), 0, c->stream, src, (const float*)c->ls_tgt,
                       (const uint8_t*)c->ls_mask, c->ls_grad + (size_t)(stage - 1) * npix * N_CH, npix, fh * fw,
                       ldexpf((float)(2.0 / ((double)npix * PMX_N_PAF)), k), ldexpf((float)(2.0 / ((double)npix * PMX_N_HEAT)), k));
    PMX_HIP(hipGetLastError());
    return pmx_prof_end(c);
}

int pmx_loss_finish(pmx_ctx* c, int n_stages, int B, int fh, int fw)
{
    if (int rc = launch_final(c, 0, PMX_LOSS_SLOTS - 1, n_stages, B, fh, fw)) return rc;
    c->ls_stages = n_stages;
    if (c->lg_on) { c->lg_stages = n_stages; c->lg_B = B; c->lg_fh = fh; c->lg_fw = fw; c->lg_scale_log2 = c->opt_loss_scale_log2; }
    return PMX_OK;
}

// ------------------------------------------------------------------------------------------ targets
extern "C" int pmx_loss_set_poses(pmx_ctx* c, const double* poses, const int* n_people, int batch, int h, int w, const uint8_t* ignore_mask,
                                  double heat_sigma, double paf_width)
{
    return pmx_loss_set_poses_masked(c, poses, n_people, batch, h, w, ignore_mask, false, heat_sigma, paf_width);
}

int pmx_loss_set_poses_masked(pmx_ctx* c, const double* poses, const int* n_people, int batch, int h, int w, const uint8_t* ignore_mask,
                              bool mask_on_device, double heat_sigma, double paf_width)
{
    PMX_CHECK(c && n_people, PMX_ERR_INVALID, "pmx_loss_set_poses: null arg");
    LOSS_POSENET(c, "pmx_loss_set_poses");
    if (int rc = check_common(c, "pmx_loss_set_poses", batch, h, w)) return rc;
    PMX_CHECK(heat_sigma > 0 && isfinite(heat_sigma), PMX_ERR_INVALID, "pmx_loss_set_poses: heat_sigma %g must be > 0", heat_sigma);
    PMX_CHECK(paf_width >= 0 && isfinite(paf_width), PMX_ERR_INVALID, "pmx_loss_set_poses: paf_width %g must be >= 0", paf_width);
    std::vector<int> off(batch + 1, 0);
    for (int b = 0; b < batch; ++b) {
        PMX_CHECK(n_people[b] >= 0 && n_people[b] < (1 << 20), PMX_ERR_INVALID, "pmx_loss_set_poses: n_people[%d] = %d", b, n_people[b]);
        off[b + 1] = off[b] + n_people[b];
        PMX_CHECK(off[b + 1] < (1 << 24), PMX_ERR_INVALID, "pmx_loss_set_poses: more than 2^24 people");
    }
    const int total = off[batch];
    PMX_CHECK(poses || total == 0, PMX_ERR_INVALID, "pmx_loss_set_poses: null poses");
    for (int p = 0; p < total; ++p)
        for (int j = 0; j < PMX_N_JOINTS; ++j) {
            const double* q = poses + (size_t)p * POSE_D + j * 3;
            PMX_CHECK(!(q[2] > 0) || (isfinite(q[0]) && isfinite(q[1])), PMX_ERR_INVALID,
                      "pmx_loss_set_poses: person %d joint %d is visible at a non-finite position", p, j);
        }
    PMX_DEV(c);
    const int fh = h / 8, fw = w / 8;
    int rc;
    if ((rc = ensure_target_buffers(c)) || (rc = ensure_grid(c, h, w))) return rc;
    if ((rc = c->ls_poses.ensure((size_t)total * POSE_D, c->stream)) || (rc = c->ls_off.ensure((size_t)c->max_batch + 1, c->stream))) return rc;
    if (ignore_mask && !mask_on_device && (rc = c->ls_mask_in.ensure((size_t)batch * h * w, c->stream))) return rc;
    c->ls_B = 0; c->ls_have_poses = false;                  // until everything below is enqueued
    c->ls_h_off = off;
    c->ls_h_poses.assign(poses, poses + (size_t)total * POSE_D);
    if (total) PMX_HIP(hipMemcpyAsync(c->ls_poses, c->ls_h_poses.data(), (size_t)total * POSE_D * sizeof(double), hipMemcpyHostToDevice, c->stream));
    PMX_HIP(hipMemcpyAsync(c->ls_off, c->ls_h_off.data(), (size_t)(batch + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (ignore_mask && !mask_on_device) {      // staged like the poses: the caller's array is read here, whatever kind of memory it is
        c->ls_h_mask.assign(ignore_mask, ignore_mask + (size_t)batch * h * w);
        PMX_HIP(hipMemcpyAsync(c->ls_mask_in, c->ls_h_mask.data(), c->ls_h_mask.size(), hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = pmx_prof_begin(c, "loss_labels|pmx_labels", (double)batch * fh * fw * (N_CH * 4 + 1)))) return rc;
    hipLaunchKernelGGL(loss_targets_kernel, dim3(blocks_for((long long)fh * fw), PMX_N_LIMBS + PMX_N_HEAT + 1, batch), dim3(256), 0, c->stream,
                       (const double*)c->ls_poses, (const int*)c->ls_off, grid_view(c), !ignore_mask ? nullptr : mask_on_device ? ignore_mask : (const uint8_t*)c->ls_mask_in,
                       (float*)c->ls_tgt, (uint8_t*)c->ls_mask, h, w, fh, fw, heat_sigma * heat_sigma, paf_width);
    PMX_HIP(hipGetLastError());
    if ((rc = pmx_prof_end(c))) return rc;
    c->ls_sigma = heat_sigma; c->ls_width = paf_width;
    c->ls_B = batch; c->ls_h = h; c->ls_w = w; c->ls_have_poses = true;
    return PMX_OK;
}

extern "C" int pmx_loss_set_targets(pmx_ctx* c, const float* paf_t, const float* heat_t, const uint8_t* ignore_mask, int batch, int th, int tw,
                                    int h, int w)
{
    PMX_CHECK(c && paf_t && heat_t, PMX_ERR_INVALID, "pmx_loss_set_targets: null arg");
    LOSS_POSENET(c, "pmx_loss_set_targets");
    if (int rc = check_common(c, "pmx_loss_set_targets", batch, h, w)) return rc;
    const int fh = h / 8, fw = w / 8;
    const bool full = th == h && tw == w;
    PMX_CHECK(full || (th == fh && tw == fw), PMX_ERR_INVALID, "pmx_loss_set_targets: maps of %d x %d are neither the input size %d x %d nor %d x %d",
              th, tw, h, w, fh, fw);
    PMX_DEV(c);
    int rc;
    if ((rc = ensure_target_buffers(c))) return rc;
    const size_t fhw = (size_t)fh * fw, hw = (size_t)h * w;
    if (full) {
        if ((rc = ensure_grid(c, h, w)) || (rc = c->ls_full.ensure(N_CH * hw, c->stream))) return rc;
        if (ignore_mask && (rc = c->ls_mask_in.ensure(batch * hw, c->stream))) return rc;
    }
    c->ls_B = 0; c->ls_have_poses = false;
    if (full) {
        // image after image through the one full-resolution staging buffer (stream-ordered: an upload waits for the launch before it)
        if (ignore_mask) PMX_HIP(hipMemcpyAsync(c->ls_mask_in, ignore_mask, batch * hw, hipMemcpyHostToDevice, c->stream));
        for (int b = 0; b < batch; ++b) {
            PMX_HIP(hipMemcpyAsync(c->ls_full, paf_t + b * PMX_N_PAF * hw, PMX_N_PAF * hw * sizeof(float), hipMemcpyHostToDevice, c->stream));
            PMX_HIP(hipMemcpyAsync(c->ls_full + PMX_N_PAF * hw, heat_t + b * PMX_N_HEAT * hw, PMX_N_HEAT * hw * sizeof(float), hipMemcpyHostToDevice,
                                   c->stream));
            hipLaunchKernelGGL(loss_resize_kernel, dim3(blocks_for((long long)fhw), N_CH + 1), dim3(256), 0, c->stream, (const float*)c->ls_full,
                               grid_view(c), ignore_mask ? (const uint8_t*)c->ls_mask_in : nullptr, (float*)c->ls_tgt, (uint8_t*)c->ls_mask, b,
                               h, w, fh, fw);
            PMX_HIP(hipGetLastError());
        }
        PMX_HIP(hipStreamSynchronize(c->stream));          // a setup call: the caller's maps may go once it returns
    } else {
        std::vector<float> t(batch * fhw * N_CH);
        std::vector<uint8_t> m(batch * fhw, 0);
        for (int b = 0; b < batch; ++b)
            for (size_t p = 0; p < fhw; ++p) {
                float* q = &t[(b * fhw + p) * N_CH];
                for (int ch = 0; ch < PMX_N_PAF; ++ch) q[ch] = paf_t[(b * PMX_N_PAF + ch) * fhw + p];
                for (int ch = 0; ch < PMX_N_HEAT; ++ch) q[PMX_N_PAF + ch] = heat_t[(b * PMX_N_HEAT + ch) * fhw + p];
                if (ignore_mask) m[b * fhw + p] = ignore_mask[b * fhw + p] ? 1 : 0;
            }
        PMX_HIP(hipMemcpyAsync(c->ls_tgt, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        PMX_HIP(hipMemcpyAsync(c->ls_mask, m.data(), m.size(), hipMemcpyHostToDevice, c->stream));
        PMX_HIP(hipStreamSynchronize(c->stream));          // the staging vectors go out of scope
    }
    c->ls_B = batch; c->ls_h = h; c->ls_w = w;
    return PMX_OK;
}

extern "C" int pmx_loss_enable(pmx_ctx* c, int on)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    LOSS_POSENET(c, "pmx_loss_enable");
    c->ls_on = on != 0;
    return PMX_OK;
}

extern "C" int pmx_loss_grad_enable(pmx_ctx* c, int on)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    LOSS_POSENET(c, "pmx_loss_grad_enable");
    if (on) {           // six stages at the context's capacity, allocated by the first use of the feature
        PMX_DEV(c);
        const size_t npix = (size_t)c->max_batch * ((size_t)c->max_h * c->max_w / 64);
        if (int rc = c->ls_grad.ensure((PMX_LOSS_SLOTS - 1) * npix * N_CH, c->stream)) return rc;
    }
    c->lg_on = on != 0;
    if (!on) c->lg_stages = 0;
    return PMX_OK;
}

extern "C" int pmx_get_loss_grads(pmx_ctx* c, int stage, float* gpaf, float* gheat)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    LOSS_POSENET(c, "pmx_get_loss_grads");
    PMX_CHECK(stage >= 0 && stage < PMX_LOSS_SLOTS - 1, PMX_ERR_INVALID, "pmx_get_loss_grads: stage %d outside 0..%d", stage, PMX_LOSS_SLOTS - 2);
    PMX_CHECK(c->lg_on && c->lg_stages > 0, PMX_ERR_STATE,
              "pmx_get_loss_grads: no forward with the validation-loss hook and the gradients on yet (pmx_loss_enable, pmx_loss_grad_enable)");
    PMX_CHECK(stage < c->lg_stages, PMX_ERR_STATE, "pmx_get_loss_grads: stage %d: the last hooked forward ran %d stages (option \"stop_stage\")",
              stage, c->lg_stages);
    PMX_DEV(c);
    const size_t fhw = (size_t)c->lg_fh * c->lg_fw, npix = c->lg_B * fhw;
    std::vector<float> t(npix * N_CH);
    PMX_HIP(hipMemcpyAsync(t.data(), c->ls_grad + (size_t)stage * npix * N_CH, t.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    PMX_HIP(hipStreamSynchronize(c->stream));
    for (int b = 0; b < c->lg_B; ++b)
        for (size_t p = 0; p < fhw; ++p) {
            const float* q = &t[(b * fhw + p) * N_CH];
            if (gpaf) for (int ch = 0; ch < PMX_N_PAF; ++ch) gpaf[(b * PMX_N_PAF + ch) * fhw + p] = q[ch];
            if (gheat) for (int ch = 0; ch < PMX_N_HEAT; ++ch) gheat[(b * PMX_N_HEAT + ch) * fhw + p] = q[PMX_N_PAF + ch];
        }
    return PMX_OK;
}

// the "loss_scale_log2" the stored gradients carry: that of the hooked forward that wrote them, whatever the option says now
extern "C" int pmx_get_loss_grad_scale(pmx_ctx* c, int* scale_log2)
{
    PMX_CHECK(c && scale_log2, PMX_ERR_INVALID, "pmx_get_loss_grad_scale: null arg");
    LOSS_POSENET(c, "pmx_get_loss_grad_scale");
    PMX_CHECK(c->lg_on && c->lg_stages > 0, PMX_ERR_STATE,
              "pmx_get_loss_grad_scale: no forward with the validation-loss hook and the gradients on yet (pmx_loss_enable, pmx_loss_grad_enable)");
    *scale_log2 = c->lg_scale_log2;
    return PMX_OK;
}

extern "C" int pmx_loss_get(pmx_ctx* c, double* paf_loss6, double* heat_loss6, int* n_stages)
{
    PMX_CHECK(c && paf_loss6 && heat_loss6 && n_stages, PMX_ERR_INVALID, "pmx_loss_get: null arg");
    LOSS_POSENET(c, "pmx_loss_get");
    PMX_CHECK(c->ls_stages > 0, PMX_ERR_STATE, "pmx_loss_get: no forward with the validation-loss hook on yet");
    PMX_DEV(c);
    double out[2 * (PMX_LOSS_SLOTS - 1)];
    PMX_HIP(hipMemcpyAsync(out, c->ls_out, sizeof out, hipMemcpyDeviceToHost, c->stream));
    PMX_HIP(hipStreamSynchronize(c->stream));
    for (int s = 0; s < PMX_LOSS_SLOTS - 1; ++s) { paf_loss6[s] = out[2 * s]; heat_loss6[s] = out[2 * s + 1]; }
    *n_stages = c->ls_stages;
    return PMX_OK;
}

extern "C" int pmx_loss_current_maps(pmx_ctx* c, double* paf_loss, double* heat_loss)
{
    PMX_CHECK(c && paf_loss && heat_loss, PMX_ERR_INVALID, "pmx_loss_current_maps: null arg");
    LOSS_POSENET(c, "pmx_loss_current_maps");
    PMX_CHECK(c->maps_valid && c->cur_segs.empty(), PMX_ERR_STATE, "pmx_loss_current_maps: no maps of a uniform batch (forward or pmx_set_maps)");
    PMX_CHECK(c->ls_B > 0, PMX_ERR_STATE, "pmx_loss_current_maps: no targets (call pmx_loss_set_poses / pmx_loss_set_targets first)");
    PMX_CHECK(c->cur_B == c->ls_B && c->cur_fh * 8 == c->ls_h && c->cur_fw * 8 == c->ls_w, PMX_ERR_STATE,
              "pmx_loss_current_maps: maps of %d x %d x %d against targets of %d x %d x %d", c->cur_B, c->cur_fh, c->cur_fw, c->ls_B, c->ls_h / 8,
              c->ls_w / 8);
    PMX_DEV(c);
    const int B = c->cur_B, fh = c->cur_fh, fw = c->cur_fw, slot = PMX_LOSS_SLOTS - 1;
    const long long fhw = (long long)fh * fw;
    const LossSrc src = c->maps_external ? LossSrc{c->ext_paf, c->ext_heat, fhw * PMX_N_PAF, fhw * PMX_N_HEAT, 1, fhw}
                                         : LossSrc{c->cat + PMX_CAT_PAF, c->cat + PMX_CAT_HEAT, fhw * PMX_CAT_C, fhw * PMX_CAT_C, PMX_CAT_C, 1};
    int rc;
    if ((rc = launch_stage(c, "loss_current|pmx_loss", slot, src, B, fh, fw)) || (rc = launch_final(c, slot, slot + 1, slot + 1, B, fh, fw))) return rc;
    double out[2];
    PMX_HIP(hipMemcpyAsync(out, c->ls_out + 2 * slot, sizeof out, hipMemcpyDeviceToHost, c->stream));
    PMX_HIP(hipStreamSynchronize(c->stream));
    *paf_loss = out[0]; *heat_loss = out[1];
    return PMX_OK;
}

extern "C" int pmx_validate_batch(pmx_ctx* c, const uint8_t* bgr, int batch, int h, int w, int on_device, double* out13)
{
    PMX_CHECK(c && bgr && out13, PMX_ERR_INVALID, "pmx_validate_batch: null arg");
    LOSS_POSENET(c, "pmx_validate_batch");
    const int was_on = c->ls_on;
    c->ls_on = 1;
    int rc = pmx_forward_u8(c, bgr, batch, h, w, on_device);
    c->ls_on = was_on;
    if (rc) return rc;
    int n = 0;
    if ((rc = pmx_loss_get(c, out13 + 1, out13 + 7, &n))) return rc;
    double total = 0.0;
    for (int s = 0; s < 6; ++s) total += out13[1 + s] + out13[7 + s];          // :68
    out13[0] = total;
    return PMX_OK;
}

extern "C" int pmx_get_labels(pmx_ctx* c, int image, float* paf, float* heat, int h, int w)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    LOSS_POSENET(c, "pmx_get_labels");
    PMX_CHECK(c->ls_B > 0 && c->ls_have_poses, PMX_ERR_STATE, "pmx_get_labels: no poses (call pmx_loss_set_poses first)");
    PMX_CHECK(image >= 0 && image < c->ls_B, PMX_ERR_INVALID, "pmx_get_labels: image %d outside 0..%d", image, c->ls_B - 1);
    PMX_CHECK(h == c->ls_h && w == c->ls_w, PMX_ERR_INVALID, "pmx_get_labels: %d x %d is not the size of the poses, %d x %d", h, w, c->ls_h, c->ls_w);
    PMX_DEV(c);
    const size_t hw = (size_t)h * w;
    int rc;
    if ((rc = c->ls_full.ensure(N_CH * hw, c->stream))) return rc;
    const int first = c->ls_h_off[image], n = c->ls_h_off[image + 1] - first;
    if ((rc = pmx_prof_begin(c, "loss_labels_full|pmx_labels", (double)hw * N_CH * 4))) return rc;
    hipLaunchKernelGGL(loss_labels_kernel, dim3(blocks_for((long long)hw), PMX_N_LIMBS + PMX_N_HEAT), dim3(256), 0, c->stream,
                       c->ls_poses + (size_t)first * POSE_D, n, (float*)c->ls_full, h, w, c->ls_sigma * c->ls_sigma, c->ls_width);
    PMX_HIP(hipGetLastError());
    if ((rc = pmx_prof_end(c))) return rc;
    if (paf) PMX_HIP(hipMemcpyAsync(paf, c->ls_full, PMX_N_PAF * hw * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (heat) PMX_HIP(hipMemcpyAsync(heat, c->ls_full + PMX_N_PAF * hw, PMX_N_HEAT * hw * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    PMX_HIP(hipStreamSynchronize(c->stream));
    return PMX_OK;
}

extern "C" int pmx_get_loss_targets(pmx_ctx* c, float* paf_t, float* heat_t, uint8_t* mask)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    LOSS_POSENET(c, "pmx_get_loss_targets");
    PMX_CHECK(c->ls_B > 0, PMX_ERR_STATE, "pmx_get_loss_targets: no targets (call pmx_loss_set_poses / pmx_loss_set_targets first)");
    PMX_DEV(c);
    const size_t fhw = (size_t)(c->ls_h / 8) * (c->ls_w / 8), npix = c->ls_B * fhw;
    std::vector<float> t(npix * N_CH);
    PMX_HIP(hipMemcpyAsync(t.data(), c->ls_tgt, t.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (mask) PMX_HIP(hipMemcpyAsync(mask, c->ls_mask, npix, hipMemcpyDeviceToHost, c->stream));
    PMX_HIP(hipStreamSynchronize(c->stream));
    for (int b = 0; b < c->ls_B; ++b)
        for (size_t p = 0; p < fhw; ++p) {
            const float* q = &t[(b * fhw + p) * N_CH];
            if (paf_t) for (int ch = 0; ch < PMX_N_PAF; ++ch) paf_t[(b * PMX_N_PAF + ch) * fhw + p] = q[ch];
            if (heat_t) for (int ch = 0; ch < PMX_N_HEAT; ++ch) heat_t[(b * PMX_N_HEAT + ch) * fhw + p] = q[PMX_N_PAF + ch];
        }
    return PMX_OK;
}
