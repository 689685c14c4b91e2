// pmx_boxes.hip -- face / hand key points for many boxes (the loop of the reference's demo.py:30-55 over the people of a picture: a face
// crop and two hand crops per person, each through FaceNet / HandNet), batched, for the boxes of any number of images in one call:
//
//   pmx_forward_u8_boxes_images   box_gather_resize_u8_images_kernel: crop_image (pose_detector.py:401-424: zero outside the image) + the
//                             optional cv2.flip(img, 1) of a left hand (hand_detector.py:29-30) + cv2.resize to the network input, OpenCV's
//                             fixed-point INTER_LINEAR (prep.hip::resize_linear_u8_kernel's arithmetic), every crop of a chunk in one
//                             launch, straight from the full images -- no crop is materialised; then the network at batch n.  A sixth
//                             box column names the box's image; the kernel reads it through a device table (address, height, width per
//                             image) that travels in the call's staging copy.
//   pmx_keypoints_images      kp_tiles_kernel<10>: F.resize_images of the last stage to the crop's own size, the optional left / right mirror
//                             of the maps (hand_detector.py:46-47), the SciPy-order Gaussian -- pp_smooth.h, the same text as
//                             pp_peaks_fast_kernel<10> -- over a flat list of 32 x 32 tiles of crops of different sizes, each block
//                             leaving an arg-max record per (tile, channel) instead of the smoothed map; kp_merge_kernel merges the
//                             records of a crop (argmax_merge is exact) into the reference's key point, tie quirk included.
//   pmx_keypoints_boxes_images    both, in chunks of the context's batch capacity taken in box order across image borders, enqueued back
//                             to back: one upload per referenced host image, one staging copy, one D2H copy and one stream
//                             synchronisation per call.
//
//   pmx_forward_u8_boxes / pmx_keypoints_boxes
//                             the boxes of ONE image: adapters that hand the image over as a table of one, with image 0 on every box.
//                             There is one implementation (forward_boxes, keypoints_boxes) and one box layout, six columns, in this file.
//
// Bit-identity: per crop the bytes of the network input equal host crop_image (+ [:, ::-1]) + pmx_forward_u8_resized, and the key points
// equal pmx_keypoints on the same maps with the crop's size and "kp_flip_x" (tests/test_gpu_face_hand_boxes.py).  Gaussian radii other
// than 10, the reference's GPU peak branch and the "pp_generic" switch take a per-crop loop over pp_keypoints_launch instead.
#include "pmx_ctx.h"
#include "pp_smooth.h"

#include <climits>
#include <cstring>

namespace {

struct BoxDesc { int left, top, w, h, flip, img, pad1, pad2; };        // crop of image `img` (w x h from (left, top)), mirrored if flip

struct BoxImg { const uint8_t* px; int h, w; };                        // one image of a many-image call: h x w x 3 uint8 on the device

struct KpCrop {                 // one crop of pmx_keypoints_images: its up-sampling tables (device pointers into the staging buffer)
    PPTables tab;
    int h, w, tiles_x, tile0;   // output size, tiles per row, first tile in the call's flat tile list
};

// crop pixel (yy, xx) of box d, mirrored when d.flip (column xx reads crop column w - 1 - xx), 0 outside the image
__device__ __forceinline__ int box_px(const uint8_t* __restrict__ img, int img_h, int img_w, const BoxDesc& d, int yy, int xx, int c)
{
    const long long iy = (long long)d.top + yy;
    const long long ix = (long long)d.left + (d.flip ? d.w - 1 - xx : xx);
    if (iy < 0 || iy >= img_h || ix < 0 || ix >= img_w) return 0;
    return (int)img[(iy * img_w + ix) * 3 + c];
}

// one thread per output pixel (3 channels) of n crops resized to dh x dw; tables per crop [x: idx0 | idx1 | coef0 | coef1 (dw each) |
// y: the same (dh each)], pmx_make_resize_table of (dst, crop extent).  Arithmetic of prep.hip::resize_linear_u8_kernel.  Crop b reads
// image desc[b].img of the table `imgs` (index checked on the host): one launch per chunk whatever images its crops come from.
__global__ __launch_bounds__(256) void box_gather_resize_u8_images_kernel(const BoxImg* __restrict__ imgs, const BoxDesc* __restrict__ desc,
                                                                          const int* __restrict__ tabs, int n, int dh, int dw,
                                                                          uint8_t* __restrict__ dst)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long npix = (long long)n * dh * dw;
    if (i >= npix) return;
    const int x = (int)(i % dw);
    const long long t = i / dw;
    const int y = (int)(t % dh);
    const int b = (int)(t / dh);
    const BoxDesc d = desc[b];
    const BoxImg im = imgs[d.img];
    const int* xtab = tabs + (long long)b * 4 * (dw + dh);
    const int* ytab = xtab + 4 * dw;
    const int sx0 = xtab[x], sx1 = xtab[dw + x], a0 = xtab[2 * dw + x], a1 = xtab[3 * dw + x];
    const int sy0 = ytab[y], sy1 = ytab[dh + y], b0 = ytab[2 * dh + y], b1 = ytab[3 * dh + y];
    uint8_t* o = dst + i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int S0 = box_px(im.px, im.h, im.w, d, sy0, sx0, c) * a0 + box_px(im.px, im.h, im.w, d, sy0, sx1, c) * a1;
        const int S1 = box_px(im.px, im.h, im.w, d, sy1, sx0, c) * a0 + box_px(im.px, im.h, im.w, d, sy1, sx1, c) * a1;
        int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
        v = v < 0 ? 0 : (v > 255 ? 255 : v);
        o[c] = (uint8_t)v;
    }
}

// grid (tiles of the chunk, n_ch): tile list entry (crop, tile of the crop); crops [crop0, ...) are images crop - crop0 of `maps`.
// The smoothed tile is pp_smooth.h's (do_nms = keep_smoothed = 0: no pruning, nothing stored); the block leaves the arg-max record of
// its 32 x 32 outputs (row-major indices of the crop's map) at rec[tile * n_ch + ch].
template <int R>
__global__ __launch_bounds__(256) void kp_tiles_kernel(PPMaps maps, const KpCrop* __restrict__ crops, const int2* __restrict__ tiles,
                                                       int tile0, int crop0, int n_ch, ArgMax* __restrict__ rec)
{
    PP_SMOOTH_FAST_DECL(R)
    __shared__ ArgMax sred[4];

    const int tid = threadIdx.x;
    const int ch = blockIdx.y;
    const int2 tl = tiles[tile0 + blockIdx.x];
    const PPTables tab = crops[tl.x].tab;
    const int map_h = crops[tl.x].h, map_w = crops[tl.x].w, tiles_x = crops[tl.x].tiles_x;
    const int b = tl.x - crop0;
    const int ty = tl.y / tiles_x, tx = tl.y - ty * tiles_x;
    const int y0 = ty * PK_TS, x0 = tx * PK_TS;
    const int keep_smoothed = 0, do_nms = 0;
    PPBuffers buf{};

    PP_SMOOTH_FAST_BODY(R)

    ArgMax a;
    a.v = -INFINITY; a.cnt = 0; a.i0 = INT_MAX; a.i1 = INT_MAX;
    for (int i = tid; i < PK_TS * PK_TS; i += 256) {
        const int r = i / PK_TS, c = i - r * PK_TS;
        const int y = y0 + r, x = x0 + c;
        if (y < map_h && x < map_w) {
            argmax_take(a, sS[(r + 1) * SW + (c + 1)], y * map_w + x);        // (a NaN makes the record NaN: pp_smooth.h)
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        ArgMax o;
        o.v = __shfl_xor(a.v, off); o.cnt = __shfl_xor(a.cnt, off); o.i0 = __shfl_xor(a.i0, off); o.i1 = __shfl_xor(a.i1, off);
        a = argmax_merge(a, o);
    }
    if (lane == 0) sred[wave] = a;
    __syncthreads();
    if (tid == 0) {
        ArgMax r = sred[0];
        for (int w = 1; w < 4; ++w) r = argmax_merge(r, sred[w]);
        rec[(long long)(tile0 + blockIdx.x) * n_ch + ch] = r;
    }
}

// grid (n_ch, crops): merge the tile records of (crop, channel) and write the key point row exactly as pp_argmax_kernel does
__global__ __launch_bounds__(256) void kp_merge_kernel(const ArgMax* __restrict__ rec, const KpCrop* __restrict__ crops,
                                                       const int* __restrict__ tile_end, int n_ch, double thresh, double* __restrict__ out)
{
    __shared__ ArgMax sred[4];
    const int ch = blockIdx.x, k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t0 = crops[k].tile0, t1 = tile_end[k], map_w = crops[k].w;
    ArgMax a;
    a.v = -INFINITY; a.cnt = 0; a.i0 = INT_MAX; a.i1 = INT_MAX;
    for (int t = t0 + tid; t < t1; t += 256) a = argmax_merge(a, rec[(long long)t * n_ch + ch]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        ArgMax o;
        o.v = __shfl_xor(a.v, off); o.cnt = __shfl_xor(a.cnt, off); o.i0 = __shfl_xor(a.i0, off); o.i1 = __shfl_xor(a.i1, off);
        a = argmax_merge(a, o);
    }
    if (lane == 0) sred[wave] = a;
    __syncthreads();
    if (tid == 0) {
        ArgMax r = sred[0];
        for (int w = 1; w < 4; ++w) r = argmax_merge(r, sred[w]);
        double* o = out + ((long long)k * n_ch + ch) * 4;
        const bool valid = (double)r.v > thresh;        // np.float32 scalar > python float: float64 comparison
        int x = r.i0 % map_w, y = r.i0 / map_w;
        if (r.cnt >= 2) { x = r.i1 / map_w; }            // (sic) coords[1] is the SECOND maximum's row when k >= 2 (pp_argmax_kernel)
        o[0] = valid ? (double)x : 0.0;
        o[1] = valid ? (double)y : 0.0;
        o[2] = (double)r.v;
        o[3] = valid ? 1.0 : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
// key-point tables of the crops of a call: where stage_keypoints reserved them (byte offsets into the staging) and the KpCrop records,
// whose table sets stage_upload builds
struct KpStage {
    size_t crops_off = 0, tiles_off = 0, ends_off = 0, taps_off = 0;
    int n_tiles = 0, fh = 0, fw = 0;    // tiles of all crops; the maps' size
    const int* hwf = nullptr;           // the call's (h, w, flip) rows
    std::vector<int> crop_tile0;        // first tile per crop, n_tiles at the end
    std::vector<size_t> grid_off;       // per crop: its grid block (pp_tables.h)
    std::vector<KpCrop> crops;
};

// the staging of one call, built on the host, copied in one piece; offsets are bytes from the start
struct Stage {
    std::vector<char> h;
    size_t put(const void* p, size_t bytes)
    {
        const size_t off = reserve(bytes);
        if (bytes) memcpy(h.data() + off, p, bytes);
        return off;
    }
    size_t reserve(size_t bytes) { const size_t off = pmx_align_up(h.size(), 16); h.resize(off + bytes); return off; }
};

// one H2D copy of the staging; the device copy is valid for the kernels enqueued after it on the context's stream.  The table sets of
// `ks` (one taps block, a grid block per crop) are built here, where the device copy's address is known: they hold device pointers into it.
int stage_upload(pmx_ctx* c, Stage& st, KpStage* ks = nullptr)
{
    const size_t bytes = st.h.size();
    if (!bytes) return PMX_OK;
    char *pinned, *dev;
    if (int rc = c->bx.begin(bytes, c->stream, &pinned, &dev)) return rc;
    if (ks) {
        char* host = st.h.data();
        PPTables taps{};
        pmx_pp_gauss(c, host + ks->taps_off, dev + ks->taps_off, taps);
        for (size_t k = 0; k < ks->crops.size(); ++k) {
            KpCrop& kc = ks->crops[k];
            kc.tab = taps;
            pp_grid_build(ks->fh, ks->fw, kc.h, kc.w, ks->hwf[3 * k + 2], host + ks->grid_off[k], dev + ks->grid_off[k], kc.tab);
        }
        memcpy(host + ks->crops_off, ks->crops.data(), ks->crops.size() * sizeof(KpCrop));
    }
    memcpy(pinned, st.h.data(), bytes);
    return c->bx.commit(bytes, c->stream);
}

// rows of 6 ints (left, top, right, bottom, flip, image): the one box layout of this file; the image index is checked by check_box_images
int check_boxes(const int* boxes6, int n)
{
    PMX_CHECK(n >= 0, PMX_ERR_INVALID, "boxes: n = %d", n);
    PMX_CHECK(n == 0 || boxes6, PMX_ERR_INVALID, "boxes: null pointer");
    for (int i = 0; i < n; ++i) {
        const int* b = boxes6 + 6 * i;
        const long long w = (long long)b[2] - b[0], h = (long long)b[3] - b[1];
        PMX_CHECK(w >= 1 && h >= 1, PMX_ERR_INVALID, "box %d: empty (left %d, top %d, right %d, bottom %d)", i, b[0], b[1], b[2], b[3]);
        PMX_CHECK(w <= INT_MAX && h <= INT_MAX && w * h < (1ll << 31), PMX_ERR_INVALID, "box %d: extent %lld x %lld outside int32", i, w, h);
        PMX_CHECK(b[4] == 0 || b[4] == 1, PMX_ERR_INVALID, "box %d: flip must be 0 or 1 (got %d)", i, b[4]);
    }
    return PMX_OK;
}

// every box names an image of the list, and every image a box names exists (an image no box refers to is never looked at)
int check_box_images(const pmx_box_image* images, int n_images, const int* boxes6, int n)
{
    PMX_CHECK(n_images >= 1 && images, PMX_ERR_INVALID, "boxes: %d images for %d boxes", images ? n_images : 0, n);
    for (int i = 0; i < n; ++i) {
        const int k = boxes6[6 * i + 5];
        PMX_CHECK(k >= 0 && k < n_images, PMX_ERR_INVALID, "box %d: image index %d outside 0..%d", i, k, n_images - 1);
        PMX_CHECK(images[k].bgr && images[k].h >= 1 && images[k].w >= 1, PMX_ERR_INVALID, "image %d (of box %d): %s, %d x %d", k, i,
                  images[k].bgr ? "bad size" : "null pointer", images[k].h, images[k].w);
    }
    return PMX_OK;
}

// the rows of a one-image entry (left, top, right, bottom, flip) in this file's layout: image 0 on every box
int boxes_of_image0(const int* boxes, int n, std::vector<int>* boxes6)
{
    PMX_CHECK(n >= 0, PMX_ERR_INVALID, "boxes: n = %d", n);
    PMX_CHECK(n == 0 || boxes, PMX_ERR_INVALID, "boxes: null pointer");
    boxes6->assign(6 * (size_t)n, 0);
    for (int i = 0; i < n; ++i) memcpy(boxes6->data() + 6 * (size_t)i, boxes + 5 * (size_t)i, 5 * sizeof(int));
    return PMX_OK;
}

// gather + resize tables of n boxes (staged) -> offsets of the descriptors and tables
void stage_boxes(Stage& st, const int* boxes6, int n, int dh, int dw, size_t* desc_off, size_t* tab_off)
{
    std::vector<BoxDesc> d(n);
    std::vector<int> tabs((size_t)n * 4 * (dw + dh));
    for (int i = 0; i < n; ++i) {
        const int* b = boxes6 + 6 * i;
        d[i] = BoxDesc{b[0], b[1], b[2] - b[0], b[3] - b[1], b[4], b[5], 0, 0};
        int* t = tabs.data() + (size_t)i * 4 * (dw + dh);
        pmx_make_resize_table(dw, d[i].w, t);
        pmx_make_resize_table(dh, d[i].h, t + 4 * dw);
    }
    *desc_off = st.put(d.data(), d.size() * sizeof(BoxDesc));
    *tab_off = st.put(tabs.data(), tabs.size() * sizeof(int));
}

// key-point tables of n crops (h, w, flip) on maps of fh x fw: the flat tile list and the per-crop tile ends are staged, room for the taps,
// a grid per crop and the KpCrop[n] records is reserved
void stage_keypoints(Stage& st, const int* hwf, int n, int fh, int fw, KpStage* ks)
{
    std::vector<int2> tiles;
    std::vector<int> ends(n);
    ks->hwf = hwf; ks->fh = fh; ks->fw = fw;
    ks->taps_off = st.reserve(pp_taps_bytes());
    ks->grid_off.resize(n);
    ks->crops.resize(n);
    ks->crop_tile0.resize(n + 1);
    for (int k = 0; k < n; ++k) {
        const int h = hwf[3 * k], w = hwf[3 * k + 1];
        ks->grid_off[k] = st.reserve(pp_grid_bytes(h, w));
        const int tx = (w + PK_TS - 1) / PK_TS, ty = (h + PK_TS - 1) / PK_TS;
        KpCrop& kc = ks->crops[k];
        kc.h = h; kc.w = w; kc.tiles_x = tx; kc.tile0 = ks->crop_tile0[k] = (int)tiles.size();
        for (int t = 0; t < tx * ty; ++t) tiles.push_back(make_int2(k, t));
        ends[k] = (int)tiles.size();
    }
    ks->n_tiles = ks->crop_tile0[n] = (int)tiles.size();
    ks->crops_off = st.reserve(n * sizeof(KpCrop));
    ks->tiles_off = st.put(tiles.data(), tiles.size() * sizeof(int2));
    ks->ends_off = st.put(ends.data(), ends.size() * sizeof(int));
}

bool kp_fast(pmx_ctx* c)
{
    return c->gauss.size() == 21 && !c->opt_gpu_branch_peaks && !c->opt_pp_generic;
}

// key points of crops [k0, k0 + B) of the call, on the current maps (images 0 .. B - 1): enqueue only
int kp_enqueue_chunk(pmx_ctx* c, const KpStage& ks, const int* hwf, int k0, int B, double thresh)
{
    const int n_ch = c->n_heat - 1;
    const PPMaps m = pmx_current_maps(c);
    int rc;
    if (kp_fast(c)) {
        const int t0 = ks.crop_tile0[k0], t1 = ks.crop_tile0[k0 + B];
        if ((rc = pmx_prof_begin(c, "kp_boxes|kp_tiles_kernel", (double)m.sbh * 4 * B))) return rc;
        hipLaunchKernelGGL(kp_tiles_kernel<10>, dim3(t1 - t0, n_ch), dim3(256), 0, c->stream, m,
                           reinterpret_cast<const KpCrop*>(c->bx.dev + ks.crops_off), reinterpret_cast<const int2*>(c->bx.dev + ks.tiles_off),
                           t0, k0, n_ch, reinterpret_cast<ArgMax*>(c->bx_rec.get()));
        PMX_HIP(hipGetLastError());
        return pmx_prof_end(c);
    }
    // fallback: one crop at a time through the post-process's own key-point launch (tables per crop, smoothed map materialised)
    for (int k = k0; k < k0 + B; ++k) {
        const int h = hwf[3 * k], w = hwf[3 * k + 1], flip = hwf[3 * k + 2];
        if ((rc = pmx_ensure_tables(c, c->cur_fh, c->cur_fw, h, w, flip))) return rc;
        if ((rc = pmx_ensure_smoothed(c, (size_t)n_ch * h * w))) return rc;
        PPMaps mk = m;
        mk.heat = m.heat + (long long)(k - k0) * m.sbh;
        if ((rc = pp_keypoints_launch(mk, c->tab, c->pp, 1, n_ch, h, w, thresh, c->d_kp + (size_t)k * n_ch * 4, c->opt_pp_generic, c->stream))) return rc;
    }
    return PMX_OK;
}

// the key-point half of a call for n crops (h, w, flip) on maps of fh x fw: checks, staging, device buffers
int kp_prepare(pmx_ctx* c, Stage& st, const int* hwf, int n, int fh, int fw, KpStage* ks)
{
    const int n_ch = c->n_heat - 1;
    int rc;
    for (int k = 0; k < n; ++k)
        PMX_CHECK(hwf[3 * k] >= 1 && hwf[3 * k + 1] >= 1 && (long long)hwf[3 * k] * hwf[3 * k + 1] < (1ll << 31) &&
                  (hwf[3 * k + 2] == 0 || hwf[3 * k + 2] == 1), PMX_ERR_INVALID, "key points: crop %d has a bad (h, w, flip) = (%d, %d, %d)",
                  k, hwf[3 * k], hwf[3 * k + 1], hwf[3 * k + 2]);
    stage_keypoints(st, hwf, n, fh, fw, ks);
    const size_t nkp = (size_t)n * n_ch * 4;
    if ((rc = c->d_kp.ensure(nkp, c->stream))) return rc;
    if (kp_fast(c) && (rc = c->bx_rec.ensure((size_t)ks->n_tiles * n_ch * sizeof(ArgMax), c->stream))) return rc;
    return PMX_OK;
}

int kp_finish(pmx_ctx* c, const KpStage& ks, int n, double thresh, double* out)
{
    const int n_ch = c->n_heat - 1;
    int rc;
    if (kp_fast(c)) {
        if ((rc = pmx_prof_begin(c, "kp_boxes|kp_merge_kernel", (double)ks.n_tiles * n_ch * sizeof(ArgMax)))) return rc;
        hipLaunchKernelGGL(kp_merge_kernel, dim3(n_ch, n), dim3(256), 0, c->stream, reinterpret_cast<const ArgMax*>(c->bx_rec.get()),
                           reinterpret_cast<const KpCrop*>(c->bx.dev + ks.crops_off), reinterpret_cast<const int*>(c->bx.dev + ks.ends_off),
                           n_ch, thresh, c->d_kp.get());
        PMX_HIP(hipGetLastError());
        if ((rc = pmx_prof_end(c))) return rc;
    }
    PMX_HIP(hipMemcpyAsync(out, c->d_kp, (size_t)n * n_ch * 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PMX_HIP(hipStreamSynchronize(c->stream));
    return PMX_OK;
}

// the image table of a call, staged (-> *imgs_off), and the uploads it needs: host images that a box refers to get a place in u8_src
// (64-bit byte offsets, 256-aligned), device images are used where they are
struct ImageCopy { size_t off; const uint8_t* src; size_t bytes; };

int stage_images(pmx_ctx* c, Stage& st, const pmx_box_image* images, int n_images, int on_device, const int* boxes6, int n,
                 size_t* imgs_off, std::vector<ImageCopy>* copies)
{
    std::vector<char> used(n_images, 0);
    for (int i = 0; i < n; ++i) used[boxes6[6 * i + 5]] = 1;
    size_t total = 0;
    copies->clear();
    if (!on_device)
        for (int k = 0; k < n_images; ++k)
            if (used[k]) {
                const size_t bytes = (size_t)images[k].h * images[k].w * 3;
                copies->push_back(ImageCopy{total, images[k].bgr, bytes});
                total += pmx_align_up(bytes, 256);
            }
    int rc;
    if (total && (rc = c->u8_src.ensure(total, c->stream))) return rc;
    std::vector<BoxImg> tab(n_images, BoxImg{nullptr, 0, 0});
    size_t next = 0;
    for (int k = 0; k < n_images; ++k)
        if (used[k]) tab[k] = BoxImg{on_device ? images[k].bgr : c->u8_src + (*copies)[next++].off, images[k].h, images[k].w};
    *imgs_off = st.put(tab.data(), tab.size() * sizeof(BoxImg));
    return PMX_OK;
}

// one copy per referenced host image, back to back on the context's stream: nothing waits in between
int upload_images(pmx_ctx* c, const std::vector<ImageCopy>& copies)
{
    for (const ImageCopy& cp : copies) PMX_HIP(hipMemcpyAsync(c->u8_src + cp.off, cp.src, cp.bytes, hipMemcpyHostToDevice, c->stream));
    if (!copies.empty()) c->pr_src = nullptr;      // (u8_src no longer holds a detect_precise original)
    return PMX_OK;
}

// gather + resize of boxes [k0, k0 + B) into u8_tmp, then the network
int forward_chunk(pmx_ctx* c, size_t imgs_off, size_t desc_off, size_t tab_off, int k0, int B)
{
    const int dh = c->max_h, dw = c->max_w;
    int rc;
    const long long npix = (long long)B * dh * dw;
    if ((rc = pmx_prof_begin(c, "resize_boxes|box_gather_resize_u8_images_kernel", (double)npix * 3 * 2))) return rc;
    hipLaunchKernelGGL(box_gather_resize_u8_images_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, c->stream,
                       reinterpret_cast<const BoxImg*>(c->bx.dev + imgs_off), reinterpret_cast<const BoxDesc*>(c->bx.dev + desc_off) + k0,
                       reinterpret_cast<const int*>(c->bx.dev + tab_off) + (size_t)k0 * 4 * (dw + dh), B, dh, dw, c->u8_tmp.get());
    PMX_HIP(hipGetLastError());
    if ((rc = pmx_prof_end(c))) return rc;
    return pmx_forward_u8(c, c->u8_tmp, B, dh, dw, 1);
}

// the two forward entries once the context and n in 1 .. max_batch are checked
int forward_boxes(pmx_ctx* c, const pmx_box_image* images, int n_images, int on_device, const int* boxes6, int n)
{
    int rc;
    if ((rc = check_boxes(boxes6, n))) return rc;
    if ((rc = check_box_images(images, n_images, boxes6, n))) return rc;
    PMX_DEV(c);
    Stage st;
    size_t desc_off, tab_off, imgs_off;
    std::vector<ImageCopy> copies;
    stage_boxes(st, boxes6, n, c->max_h, c->max_w, &desc_off, &tab_off);
    if ((rc = stage_images(c, st, images, n_images, on_device, boxes6, n, &imgs_off, &copies))) return rc;
    if ((rc = upload_images(c, copies))) return rc;
    if ((rc = stage_upload(c, st))) return rc;
    return forward_chunk(c, imgs_off, desc_off, tab_off, 0, n);
}

// the two one-call entries once the context is checked
int keypoints_boxes(pmx_ctx* c, const pmx_box_image* images, int n_images, int on_device, const int* boxes6, int n, double thresh,
                    double* out)
{
    int rc;
    if ((rc = check_boxes(boxes6, n))) return rc;
    if (n == 0) return PMX_OK;
    if ((rc = check_box_images(images, n_images, boxes6, n))) return rc;
    PMX_CHECK(out, PMX_ERR_INVALID, "boxes: null output");
    if ((rc = pmx_check_weights(c))) return rc;
    PMX_DEV(c);
    const int fh = c->max_h / 8, fw = c->max_w / 8;      // the maps of a max_h x max_w input: those of the forwards below
    std::vector<int> hwf(3 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        const int* b = boxes6 + 6 * i;
        hwf[3 * i] = b[3] - b[1]; hwf[3 * i + 1] = b[2] - b[0]; hwf[3 * i + 2] = b[4];
    }
    Stage st;
    size_t desc_off, tab_off, imgs_off;
    std::vector<ImageCopy> copies;
    KpStage ks;
    stage_boxes(st, boxes6, n, c->max_h, c->max_w, &desc_off, &tab_off);
    if ((rc = kp_prepare(c, st, hwf.data(), n, fh, fw, &ks))) return rc;
    if ((rc = stage_images(c, st, images, n_images, on_device, boxes6, n, &imgs_off, &copies))) return rc;
    if ((rc = upload_images(c, copies))) return rc;
    if ((rc = stage_upload(c, st, &ks))) return rc;
    for (int k0 = 0; k0 < n; k0 += c->max_batch) {       // chunks in box order, across image borders
        const int B = n - k0 < c->max_batch ? n - k0 : c->max_batch;
        if ((rc = forward_chunk(c, imgs_off, desc_off, tab_off, k0, B))) return rc;
        PMX_CHECK(c->cur_fh == fh && c->cur_fw == fw, PMX_ERR_STATE, "boxes: maps of %d x %d, expected %d x %d", c->cur_fh, c->cur_fw, fh, fw);
        if ((rc = kp_enqueue_chunk(c, ks, hwf.data(), k0, B, thresh))) return rc;
    }
    return kp_finish(c, ks, n, thresh, out);
}

}  // namespace

extern "C" int pmx_keypoints_images(pmx_ctx* c, int B, const int* hwf, double thresh, double* out)
{
    PMX_CHECK(c && hwf && out, PMX_ERR_INVALID, "null arg");
    PMX_CHECK(c->kind != NET_POSE, PMX_ERR_STATE, "pmx_keypoints_images: facenet / handnet only");
    PMX_CHECK(c->maps_valid && B == c->cur_B && B >= 1, PMX_ERR_STATE, "pmx_keypoints_images: no network output for batch %d", B);
    PMX_CHECK(c->cur_segs.empty(), PMX_ERR_STATE, "pmx_keypoints_images: the current maps are those of a mixed-size batch");
    PMX_DEV(c);
    int rc;
    Stage st;
    KpStage ks;
    if ((rc = kp_prepare(c, st, hwf, B, c->cur_fh, c->cur_fw, &ks))) return rc;
    if ((rc = stage_upload(c, st, &ks))) return rc;
    if ((rc = kp_enqueue_chunk(c, ks, hwf, 0, B, thresh))) return rc;
    return kp_finish(c, ks, B, thresh, out);
}

extern "C" int pmx_forward_u8_boxes_images(pmx_ctx* c, const pmx_box_image* images, int n_images, int on_device, const int* boxes6, int n)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    PMX_CHECK(c->kind != NET_POSE, PMX_ERR_STATE, "pmx_forward_u8_boxes_images: facenet / handnet only");
    PMX_CHECK(n >= 1 && n <= c->max_batch, PMX_ERR_CAPACITY, "pmx_forward_u8_boxes_images: %d boxes outside 1..%d", n, c->max_batch);
    return forward_boxes(c, images, n_images, on_device, boxes6, n);
}

extern "C" int pmx_keypoints_boxes_images(pmx_ctx* c, const pmx_box_image* images, int n_images, int on_device, const int* boxes6, int n,
                                          double thresh, double* out)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    PMX_CHECK(c->kind != NET_POSE, PMX_ERR_STATE, "pmx_keypoints_boxes_images: facenet / handnet only");
    return keypoints_boxes(c, images, n_images, on_device, boxes6, n, thresh, out);
}

// ---- the one-image entries: the image as a table of one, image 0 on every box
extern "C" int pmx_forward_u8_boxes(pmx_ctx* c, const uint8_t* img, int img_h, int img_w, int on_device, const int* boxes, int n)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    PMX_CHECK(c->kind != NET_POSE, PMX_ERR_STATE, "pmx_forward_u8_boxes: facenet / handnet only");
    PMX_CHECK(n >= 1 && n <= c->max_batch, PMX_ERR_CAPACITY, "pmx_forward_u8_boxes: %d boxes outside 1..%d", n, c->max_batch);
    int rc;
    std::vector<int> boxes6;
    if ((rc = boxes_of_image0(boxes, n, &boxes6))) return rc;
    const pmx_box_image image{img, img_h, img_w};
    return forward_boxes(c, &image, 1, on_device, boxes6.data(), n);
}

extern "C" int pmx_keypoints_boxes(pmx_ctx* c, const uint8_t* img, int img_h, int img_w, int on_device, const int* boxes, int n,
                                   double thresh, double* out)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    PMX_CHECK(c->kind != NET_POSE, PMX_ERR_STATE, "pmx_keypoints_boxes: facenet / handnet only");
    int rc;
    std::vector<int> boxes6;
    if ((rc = boxes_of_image0(boxes, n, &boxes6))) return rc;
    const pmx_box_image image{img, img_h, img_w};
    return keypoints_boxes(c, &image, 1, on_device, boxes6.data(), n, thresh, out);
}
