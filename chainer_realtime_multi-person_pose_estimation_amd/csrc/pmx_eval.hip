// pmx_eval.hip -- COCO key-point evaluation per image on the device: the stable score ranking and the cut to 20 detections, the
// detections' areas, the OKS matrix in fp64 and the 3 area ranges x 10 thresholds greedy matching walks of COCOeval's evaluateImg.  The
// contract is the package's own host functions (coco.py: oks_matrix / evaluate_image); include/pose_mi355x.h (pmx_coco_eval) writes it
// out.  Compiled with -ffp-contract=off: every double product and sum below is rounded on its own, as NumPy rounds it; fp64 division is
// correctly rounded.  The one operation that differs from the host is exp (about one ulp on either side).
//
//   eval_kernel   ONE launch per call, one block per image.  The image's working set lives in LDS (ev_lds_bytes: 208 bytes per ground
//                 truth + 5840): the OKS matrix, the ground truths' areas and flags, their visiting order per area range, the ranked
//                 detections' points, and a row of matched flags per walk.  Steps, a barrier between each: (1) a lane per person counts
//                 the people that rank before it (higher score, or equal score and earlier) -- its rank, written if below 20; a lane per
//                 ground truth reads its area and flags; (2) a lane per (detection, key point) picks the COCO point out of the pose;
//                 (3) a lane per detection takes the bounding area; a lane per (ground truth, detection) sums its OKS terms in key-point
//                 order; three lanes build gt_ig and the kept-first order of their range; (4) thirty lanes walk their (range, threshold)
//                 -- the walks share nothing but read-only tables; (5) everything is written out.  No atomics.
// Detections come from the caller's arrays or from the result records where the post-process left them (pmx_image_info | scores[cap] |
// poses[cap][18][3]); the kernel reads n_people of a record itself, so the host never sees a pose.
#include "pmx_ctx.h"

#include <cmath>
#include <cstring>

namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_D = PMX_EVAL_MAX_DETS, EV_K = PMX_EVAL_KEYPOINTS, EV_T = 10, EV_A = 3;

struct EvImg { int gt0, n_gt, person0, n_people; long long out_gt0; };
static_assert(sizeof(EvImg) == 24, "EvImg layout");
static_assert(sizeof(pmx_eval_gt) == 456 && sizeof(pmx_eval_consts) == 344, "pmx_eval table layout");

struct EvArgs {
    const EvImg* imgs; const pmx_eval_gt* gts; const pmx_eval_consts* k;
    const double* poses; const double* scores;                          // form 1
    const unsigned char* records; size_t rec_bytes; int cap_ppl;        // form 2 (records != null)
    int* det_count; int* det_order; double* det_scores; double* det_areas; int* dt_match; uint8_t* dt_ig; uint8_t* gt_ig;
    double* oks;                                                         // null: not asked for
};

// the LDS of an image with G ground truths (the derivation of PMX_EVAL_MAX_GT in the header)
__host__ __device__ constexpr size_t ev_lds_bytes(int G)
{
    return sizeof(double) * ((size_t)(EV_D + 1) * G + 2 * EV_D * EV_K + 2 * EV_D) + sizeof(int) * EV_D + (size_t)G * (2 * EV_A + EV_A + 1 + EV_A * EV_T);
}
static_assert(ev_lds_bytes(PMX_EVAL_MAX_GT) <= 160 * 1024 && ev_lds_bytes(PMX_EVAL_MAX_GT * 3 / 2) > 160 * 1024, "PMX_EVAL_MAX_GT against 160 KB of LDS");

__global__ __launch_bounds__(EV_THREADS) void eval_kernel(EvArgs a)
{
    extern __shared__ double ev_lds[];
    const int img = (int)blockIdx.x, tid = (int)threadIdx.x;
    const EvImg im = a.imgs[img];
    const int G = im.n_gt;
    const pmx_eval_consts& K = *a.k;
    const pmx_eval_gt* gts = a.gts + im.gt0;
    double* s_oks = ev_lds;                                            // [EV_D][G]
    double* s_garea = s_oks + (size_t)EV_D * G;                        // [G]
    double* s_dx = s_garea + G;                                        // [EV_D][EV_K]
    double* s_dy = s_dx + EV_D * EV_K;
    double* s_dscore = s_dy + EV_D * EV_K;                             // [EV_D]
    double* s_darea = s_dscore + EV_D;
    int* s_dorder = reinterpret_cast<int*>(s_darea + EV_D);            // [EV_D]
    unsigned short* s_gorder = reinterpret_cast<unsigned short*>(s_dorder + EV_D);      // [EV_A][G]
    unsigned char* s_gig = reinterpret_cast<unsigned char*>(s_gorder + (size_t)EV_A * G);   // [EV_A][G]
    unsigned char* s_gflag = s_gig + (size_t)EV_A * G;                 // [G]: bit 0 crowd, bit 1 ignore
    unsigned char* s_matched = s_gflag + G;                            // [EV_A * EV_T][G]

    int n;
    const double *sc, *ps;
    if (a.records) {
        const unsigned char* rec = a.records + (size_t)img * a.rec_bytes;
        n = reinterpret_cast<const pmx_image_info*>(rec)->n_people;
        n = n < 0 ? 0 : n > a.cap_ppl ? a.cap_ppl : n;
        sc = reinterpret_cast<const double*>(rec + sizeof(pmx_image_info));
        ps = sc + a.cap_ppl;
    } else {
        n = im.n_people;
        sc = a.scores + im.person0;
        ps = a.poses + (size_t)im.person0 * (PMX_N_JOINTS * 3);
    }
    const int D = n < EV_D ? n : EV_D;

    // (1) ranks: argsort(-score, kind='mergesort') cut to EV_D; the ground truths' areas and flags.  Finite scores give every rank
    // 0 .. n - 1 once; a NaN in a record could leave a rank out, and that slot then names person 0 instead of nobody.
    if (tid < EV_D) s_dorder[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += EV_THREADS) {
        const double si = sc[i];
        int r = 0;
        for (int j = 0; j < n; ++j) {
            const double sj = sc[j];
            r += (sj > si || (sj == si && j < i)) ? 1 : 0;
        }
        if (r < EV_D) s_dorder[r] = i;
    }
    for (int g = tid; g < G; g += EV_THREADS) {
        s_garea[g] = gts[g].area;
        s_gflag[g] = (unsigned char)((gts[g].iscrowd == 1 ? 1 : 0) | ((gts[g].iscrowd == 1 || gts[g].num_keypoints == 0) ? 2 : 0));
    }
    __syncthreads();

    // (2) the COCO key points of the ranked detections
    for (int item = tid; item < D * EV_K; item += EV_THREADS) {
        const int d = item / EV_K, i = item - d * EV_K;
        const double* row = ps + ((size_t)s_dorder[d] * PMX_N_JOINTS + K.joint[i]) * 3;
        const bool found = row[2] != 0.0;
        s_dx[item] = found ? row[0] : 0.0;
        s_dy[item] = found ? row[1] : 0.0;
    }
    if (tid < D) s_dscore[tid] = sc[s_dorder[tid]];
    __syncthreads();

    // (3) areas, OKS, gt_ig and the visiting orders
    if (tid < D) {
        double x0 = s_dx[tid * EV_K], x1 = x0, y0 = s_dy[tid * EV_K], y1 = y0;
        for (int i = 1; i < EV_K; ++i) {
            const double x = s_dx[tid * EV_K + i], y = s_dy[tid * EV_K + i];
            x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1;
            y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
        }
        s_darea[tid] = (x1 - x0) * (y1 - y0);
    }
    for (int item = tid; item < D * G; item += EV_THREADS) {
        const int g = item / D, d = item - g * D;
        const pmx_eval_gt& gt = gts[g];
        int k1 = 0;
        for (int i = 0; i < EV_K; ++i) k1 += gt.keypoints[i][2] > 0 ? 1 : 0;
        const double bx0 = gt.bbox[0] - gt.bbox[2], bx1 = gt.bbox[0] + gt.bbox[2] * 2, by0 = gt.bbox[1] - gt.bbox[3], by1 = gt.bbox[1] + gt.bbox[3] * 2;
        const double den = gt.area + K.eps;
        double sum = 0;
        int cnt = 0;
        for (int i = 0; i < EV_K; ++i) {
            const double xd = s_dx[d * EV_K + i], yd = s_dy[d * EV_K + i];
            double dx, dy;
            if (k1 > 0) {
                if (!(gt.keypoints[i][2] > 0)) continue;
                dx = xd - gt.keypoints[i][0];
                dy = yd - gt.keypoints[i][1];
            } else {
                dx = fmax(0.0, bx0 - xd) + fmax(0.0, xd - bx1);
                dy = fmax(0.0, by0 - yd) + fmax(0.0, yd - by1);
            }
            const double e = (dx * dx + dy * dy) / K.vars[i] / den / 2;
            sum += exp(-e);
            cnt += 1;
        }
        s_oks[(size_t)d * G + g] = sum / cnt;
    }
    if (tid >= EV_THREADS - EV_A) {                  // (the last lanes: the first ones carry the areas)
        const int ar = EV_THREADS - 1 - tid;
        const double lo = K.area_rngs[ar][0], hi = K.area_rngs[ar][1];
        int kept = 0;
        for (int g = 0; g < G; ++g) {
            const bool ig = (s_gflag[g] & 2) || s_garea[g] < lo || s_garea[g] > hi;
            s_gig[ar * G + g] = ig ? 1 : 0;
            kept += ig ? 0 : 1;
        }
        int pk = 0, pi = kept;                       // argsort(gt_ig, kind='mergesort'): kept ones first, file order within each group
        for (int g = 0; g < G; ++g) {
            if (s_gig[ar * G + g]) s_gorder[ar * G + pi++] = (unsigned short)g;
            else s_gorder[ar * G + pk++] = (unsigned short)g;
        }
    }
    __syncthreads();

    // (4) the walks
    if (tid < EV_A * EV_T) {
        const int ar = tid / EV_T, t = tid - ar * EV_T;
        const double lo = K.area_rngs[ar][0], hi = K.area_rngs[ar][1];
        const double thr = fmin(K.iou_thrs[t], 1 - 1e-10);
        unsigned char* mt = s_matched + (size_t)tid * G;
        const unsigned char* gig = s_gig + (size_t)ar * G;
        const unsigned short* order = s_gorder + (size_t)ar * G;
        for (int g = 0; g < G; ++g) mt[g] = 0;
        const size_t o = (((size_t)img * EV_A + ar) * EV_T + t) * EV_D;
        for (int d = 0; d < EV_D; ++d) {
            int m = -1, ig = 0;
            if (d < D) {
                double iou = thr;
                for (int q = 0; q < G; ++q) {
                    const int g = order[q];
                    if (mt[g] && !(s_gflag[g] & 1)) continue;
                    if (m > -1 && !gig[m] && gig[g]) break;
                    const double v = s_oks[(size_t)d * G + g];
                    if (v < iou) continue;
                    iou = v;
                    m = g;
                }
                if (m >= 0) { ig = gig[m]; mt[m] = 1; }
                else ig = (s_darea[d] < lo || s_darea[d] > hi) ? 1 : 0;
            }
            a.dt_match[o + d] = m;
            a.dt_ig[o + d] = (uint8_t)ig;
        }
    }

    // (5) the rest of the outputs
    if (tid == 0) a.det_count[img] = D;
    if (tid < EV_D) {
        const bool on = tid < D;
        a.det_order[(size_t)img * EV_D + tid] = on ? s_dorder[tid] : -1;
        a.det_scores[(size_t)img * EV_D + tid] = on ? s_dscore[tid] : 0.0;
        a.det_areas[(size_t)img * EV_D + tid] = on ? s_darea[tid] : 0.0;
    }
    for (int i = tid; i < EV_A * G; i += EV_THREADS) {
        const int g = i / EV_A, ar = i - g * EV_A;
        a.gt_ig[(size_t)(im.out_gt0 + g) * EV_A + ar] = s_gig[ar * G + g];
    }
    if (a.oks)
        for (int i = tid; i < EV_D * G; i += EV_THREADS) a.oks[(size_t)im.out_gt0 * EV_D + i] = i < D * G ? s_oks[i] : 0.0;
}

// everything pmx_coco_eval refuses, before anything is enqueued (the in-place form's state is checked by the caller)
int check_eval(const pmx_eval_image* images, int n_images, const pmx_eval_gt* gts, int n_gts, const pmx_eval_consts* k, const double* poses,
               const double* scores, const int32_t* n_people)
{
    PMX_CHECK(images && n_images > 0, PMX_ERR_INVALID, "coco_eval: %s", images ? "n_images <= 0" : "null image table");
    PMX_CHECK(n_gts >= 0 && (n_gts == 0 || gts), PMX_ERR_INVALID, "coco_eval: %d ground truths and a null table", n_gts);
    PMX_CHECK(k, PMX_ERR_INVALID, "coco_eval: null constant tables");
    for (int i = 0; i < EV_K; ++i) {
        PMX_CHECK(std::isfinite(k->vars[i]) && k->vars[i] > 0, PMX_ERR_INVALID, "coco_eval: vars[%d] = %g", i, k->vars[i]);
        PMX_CHECK(k->joint[i] >= 0 && k->joint[i] < PMX_N_JOINTS, PMX_ERR_INVALID, "coco_eval: joint[%d] = %d outside 0 .. %d", i, k->joint[i], PMX_N_JOINTS - 1);
    }
    for (int i = 0; i < EV_T; ++i) PMX_CHECK(std::isfinite(k->iou_thrs[i]), PMX_ERR_INVALID, "coco_eval: iou_thrs[%d] is not finite", i);
    for (int i = 0; i < EV_A; ++i)
        PMX_CHECK(std::isfinite(k->area_rngs[i][0]) && std::isfinite(k->area_rngs[i][1]), PMX_ERR_INVALID, "coco_eval: area_rngs[%d] is not finite", i);
    PMX_CHECK(std::isfinite(k->eps), PMX_ERR_INVALID, "coco_eval: eps is not finite");
    for (int im = 0; im < n_images; ++im) {
        const pmx_eval_image& e = images[im];
        PMX_CHECK(e.n_gt >= 0, PMX_ERR_INVALID, "coco_eval: image %d: %d ground truths", im, e.n_gt);
        PMX_CHECK(e.gt0 >= 0 && (long long)e.gt0 + e.n_gt <= n_gts, PMX_ERR_INVALID, "coco_eval: image %d: ground truths %d .. %d outside the table of %d", im,
                  e.gt0, e.gt0 + e.n_gt - 1, n_gts);
        for (int g = 0; g < e.n_gt; ++g) {
            const pmx_eval_gt& gt = gts[e.gt0 + g];
            bool ok = std::isfinite(gt.area);
            for (int i = 0; i < 4; ++i) ok = ok && std::isfinite(gt.bbox[i]);
            for (int i = 0; i < EV_K * 3; ++i) ok = ok && std::isfinite(gt.keypoints[0][i]);
            PMX_CHECK(ok, PMX_ERR_INVALID, "coco_eval: image %d, ground truth %d: a coordinate, the area or the box is not finite", im, g);
        }
    }
    if (poses) {
        PMX_CHECK(scores && n_people, PMX_ERR_INVALID, "coco_eval: poses without %s", scores ? "n_people" : "scores");
        size_t total = 0;
        for (int im = 0; im < n_images; ++im) {
            PMX_CHECK(n_people[im] >= 0, PMX_ERR_INVALID, "coco_eval: image %d: %d people", im, n_people[im]);
            total += (size_t)n_people[im];
        }
        for (size_t p = 0; p < total; ++p) {
            bool ok = std::isfinite(scores[p]);
            for (int i = 0; i < PMX_N_JOINTS * 3; ++i) ok = ok && std::isfinite(poses[p * (PMX_N_JOINTS * 3) + i]);
            PMX_CHECK(ok, PMX_ERR_INVALID, "coco_eval: person %zu: a coordinate or the score is not finite", p);
        }
    }
    for (int im = 0; im < n_images; ++im)
        PMX_CHECK(images[im].n_gt <= PMX_EVAL_MAX_GT, PMX_ERR_CAPACITY, "coco_eval: image %d has %d ground truths (at most PMX_EVAL_MAX_GT = %d per image)", im,
                  images[im].n_gt, PMX_EVAL_MAX_GT);
    return PMX_OK;
}

}   // namespace

extern "C" int pmx_coco_eval(pmx_ctx* c, const pmx_eval_image* images, int n_images, const pmx_eval_gt* gts, int n_gts, const pmx_eval_consts* consts,
                             const double* poses, const double* scores, const int32_t* n_people, int32_t* det_count, int32_t* det_order,
                             double* det_scores, double* det_areas, int32_t* dt_match, uint8_t* dt_ig, uint8_t* gt_ig, double* oks)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    PMX_CHECK(det_count || det_order || det_scores || det_areas || dt_match || dt_ig || gt_ig || oks, PMX_ERR_INVALID, "coco_eval: every output is null");
    int rc;
    if ((rc = check_eval(images, n_images, gts, n_gts, consts, poses, scores, n_people))) return rc;
    const bool in_place = poses == nullptr;
    if (in_place) PMX_CHECK(c->pp_valid && n_images <= c->pp_B, PMX_ERR_STATE, "coco_eval: no post-process records for %d images", n_images);

    // the layout of the ONE staging block [image table | ground truths | constants | scores | poses]
    std::vector<EvImg> tab(n_images);
    size_t people = 0, sum_gt = 0;
    int max_gt = 0;
    for (int k = 0; k < n_images; ++k) {
        tab[k] = EvImg{images[k].gt0, images[k].n_gt, (int)people, in_place ? -1 : n_people[k], (long long)sum_gt};
        if (!in_place) people += (size_t)n_people[k];
        sum_gt += (size_t)images[k].n_gt;
        max_gt = std::max(max_gt, images[k].n_gt);
    }
    PMX_CHECK(people < ((size_t)1 << 31), PMX_ERR_CAPACITY, "coco_eval: more than 2^31 people in one call");
    const size_t gt_off = pmx_align_up((size_t)n_images * sizeof(EvImg), 64);
    const size_t k_off = pmx_align_up(gt_off + (size_t)n_gts * sizeof(pmx_eval_gt), 64);
    const size_t sc_off = pmx_align_up(k_off + sizeof(pmx_eval_consts), 64);
    const size_t ps_off = pmx_align_up(sc_off + people * sizeof(double), 64);
    const size_t bytes = pmx_align_up(ps_off + people * (PMX_N_JOINTS * 3) * sizeof(double), 64);
    PMX_CHECK(bytes <= PMX_EVAL_TABLE_BYTES, PMX_ERR_CAPACITY, "coco_eval: %zu bytes of tables exceed the budget of %zu", bytes, (size_t)PMX_EVAL_TABLE_BYTES);
    // ... and of the output block
    const size_t slots = (size_t)n_images * EV_D, cells = slots * EV_A * EV_T;
    const size_t o_scores = 0, o_areas = o_scores + slots * sizeof(double), o_oks = o_areas + slots * sizeof(double);
    const size_t o_match = o_oks + (oks ? sum_gt * EV_D * sizeof(double) : 0), o_order = o_match + cells * sizeof(int);
    const size_t o_count = o_order + slots * sizeof(int), o_dtig = o_count + (size_t)n_images * sizeof(int), o_gtig = o_dtig + cells;
    const size_t out_bytes = o_gtig + sum_gt * EV_A;

    PMX_DEV(c);
    EvArgs a{};
    if (in_place) {
        int cap = 0;
        size_t rec = 0;
        if ((rc = pmx_results_layout(c, &cap, &rec))) return rc;       // final records: grows and re-runs the post-process if it must
        a.records = c->pp.results; a.rec_bytes = rec; a.cap_ppl = cap;
    }
    static std::atomic<bool> attr_set[PMX_MAX_DEVICES] = {};
    if ((rc = conv_allow_big_lds(reinterpret_cast<const void*>(eval_kernel), attr_set))) return rc;
    if ((rc = c->ev_out.ensure(out_bytes, c->stream))) return rc;
    char *host, *dev;
    if ((rc = c->ev.begin(bytes, c->stream, &host, &dev))) return rc;
    memcpy(host, tab.data(), tab.size() * sizeof(EvImg));
    if (n_gts) memcpy(host + gt_off, gts, (size_t)n_gts * sizeof(pmx_eval_gt));
    memcpy(host + k_off, consts, sizeof(pmx_eval_consts));
    if (people) {
        memcpy(host + sc_off, scores, people * sizeof(double));
        memcpy(host + ps_off, poses, people * (PMX_N_JOINTS * 3) * sizeof(double));
    }
    if ((rc = c->ev.commit(bytes, c->stream))) return rc;

    char* out = c->ev_out;
    a.imgs = reinterpret_cast<const EvImg*>(dev);
    a.gts = reinterpret_cast<const pmx_eval_gt*>(dev + gt_off);
    a.k = reinterpret_cast<const pmx_eval_consts*>(dev + k_off);
    if (!in_place) { a.scores = reinterpret_cast<const double*>(dev + sc_off); a.poses = reinterpret_cast<const double*>(dev + ps_off); }
    a.det_scores = reinterpret_cast<double*>(out + o_scores); a.det_areas = reinterpret_cast<double*>(out + o_areas);
    a.oks = oks ? reinterpret_cast<double*>(out + o_oks) : nullptr;
    a.dt_match = reinterpret_cast<int*>(out + o_match); a.det_order = reinterpret_cast<int*>(out + o_order);
    a.det_count = reinterpret_cast<int*>(out + o_count);
    a.dt_ig = reinterpret_cast<uint8_t*>(out + o_dtig); a.gt_ig = reinterpret_cast<uint8_t*>(out + o_gtig);

    if ((rc = pmx_prof_begin(c, "coco_eval|eval_kernel", (double)(bytes + out_bytes)))) return rc;
    hipLaunchKernelGGL(eval_kernel, dim3((unsigned)n_images), dim3(EV_THREADS), ev_lds_bytes(max_gt), c->stream, a);
    PMX_HIP(hipGetLastError());
    if ((rc = pmx_prof_end(c))) return rc;
    auto fetch = [&](void* dst, size_t off, size_t n) -> hipError_t {
        return dst && n ? hipMemcpyAsync(dst, out + off, n, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    };
    PMX_HIP(fetch(det_count, o_count, (size_t)n_images * sizeof(int)));
    PMX_HIP(fetch(det_order, o_order, slots * sizeof(int)));
    PMX_HIP(fetch(det_scores, o_scores, slots * sizeof(double)));
    PMX_HIP(fetch(det_areas, o_areas, slots * sizeof(double)));
    PMX_HIP(fetch(dt_match, o_match, cells * sizeof(int)));
    PMX_HIP(fetch(dt_ig, o_dtig, cells));
    PMX_HIP(fetch(gt_ig, o_gtig, sum_gt * EV_A));
    PMX_HIP(fetch(oks, o_oks, sum_gt * EV_D * sizeof(double)));
    PMX_HIP(hipStreamSynchronize(c->stream));
    return PMX_OK;
}
