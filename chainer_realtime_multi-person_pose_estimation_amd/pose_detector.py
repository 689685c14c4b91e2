"""`PoseDetector` -- drop-in mirror of the reference class (reference `pose_detector.py:15-517`) whose
hot path runs on one MI355X through libpose_mi355x.so (C ABI: include/pose_mi355x.h).

Same constructor and call signature as the reference:

    PoseDetector(arch=None, weights_file=None, model=None, device=-1, precise=False)   # pose_detector.py:16
    poses, scores = detector(orig_img)          # orig_img: H x W x 3 uint8 BGR             pose_detector.py:484

`poses` is float64 (n, 18, 3) rows [x, y, 2] / [0, 0, 0] in original-image pixels, `scores` float64 (n,);
the "nothing found" returns have the reference's shapes (:509-510, :264).  The numerics are those of the
reference's CPU branch (the golden one): SciPy-equivalent Gaussian, 4-neighbour strict NMS, NumPy-order
float64 PAF scoring, greedy matching and grouping -- executed by HIP kernels.

What `model=` means here (the reference's plug-in seam, :19-20):
  * None                -> the built-in CocoPoseNet kernels with `weights_file` (Chainer NPZ) or `weights=`;
  * dict name->(W, b)   -> the built-in kernels with these weights;
  * a callable          -> called as `model(x)` with the float32 NCHW input exactly like the reference calls its
                           Chain (:499); it must return `(pafs, heatmaps)` lists whose last elements are arrays
                           of shape (1, 38, h, w) / (1, 19, h, w).  Their values are installed on the device and
                           the post-process runs on the GPU (this is how the tests inject synthetic skeletons).

`device`: GPU index; -1 (the reference's "CPU") selects GPU 0 -- there is one numerics path (the CPU-branch
semantics) and it always runs on the MI355X; there is no CPU fallback, construction raises without a GPU.
"""
import math

import numpy as np

from . import native
from . import weights as weights_mod
from .entity import JointType, params


class PoseDetector(object):
    precise_largest_first = True      # detect_precise enqueues its largest scale first (same results: the parts are summed in the reference's order)

    def __init__(self, arch=None, weights_file=None, model=None, device=-1, precise=False, weights=None,
                 max_batch=1, max_size=None, gpu_branch_peaks=False, precision='f32'):
        self.arch = arch
        self.precise = precise
        self.device = device
        self._gpu = device if device >= 0 else 0
        self.model = None
        w = None
        if callable(model):
            self.model = model
        elif isinstance(model, dict):
            w = model
        elif model is not None:
            raise TypeError('model must be None, a weights dict or a callable returning (pafs, heatmaps)')
        else:
            if arch not in (None, 'posenet'):
                raise ValueError("only arch='posenet' is on the accelerated path (got %r)" % (arch,))
            if weights is not None:
                w = weights
            elif weights_file:
                w = weights_mod.load_npz(weights_file)     # serializers.load_npz (:26)
        size = params['inference_img_size']
        mh, mw = (size, size) if max_size is None else max_size
        self._weights = w
        self._gpu_branch_peaks = bool(gpu_branch_peaks)
        if precision not in native.PRECISIONS:
            raise ValueError("precision must be one of %s, got %r: 'f32' (default: the fp32 arithmetic the parity tests specify), 'f16' (opt-in "
                             "inference mode: 3x3 / 7x7 layers on the f16 matrix cores, f16 operands, fp32 sums; accuracy contract in "
                             "INTEGRATION.md section 4) or 'bf16x3' (opt-in, frozen: 3x3 / 7x7 layers on the bf16 matrix cores with three-term "
                             "splits, fp32-grade accuracy, SLOWER than the fp32 Winograd path since round 5; needs a library built with "
                             "PMX_BUILD_BF16X3=1)" % (', '.join(repr(p) for p in native.PRECISIONS), precision))
        self._precision = precision
        self.engine = None
        self._train_on = False                     # training mode (train_step): the optimiser's stores live in the engine
        self._trunk = False                        # set_trainable: train_step updates conv1_1 .. conv4_2 as well
        self._mode2 = False                        # training retains the trunk (engine backward mode 2); stays once the trunk was trainable
        self._adam = dict(alpha=1e-4, beta1=0.9, beta2=0.999, eps=1e-8)
        self._grad_scales = dict(self.REFERENCE_GRAD_SCALES)
        self._grad_precision = 'f32'               # set_gradient_precision: engine option "grad_precision" of the head backward
        self._loss_scale_log2 = 0                  # ... and k of the static loss scale 2^k (engine option "loss_scale_log2")
        self._make_engine(max_batch, mh, mw)

    def _make_engine(self, max_batch, mh, mw):
        # growth keeps the engine's state: weights (also those installed through detector.engine.set_weights / set_layer), options,
        # stream, capacities -- taken from the old context, which is destroyed BEFORE the larger one is created (the two never hold
        # their buffers and weight packs at the same time)
        st = opt = None
        if self.engine is not None:
            if self._train_on:                     # Adam's state moves to the larger context with the weights
                opt = self.optimizer_state()
                self._train_on = False
            st = self.engine.state()
            self.engine.close()
            self.engine = None
        try:
            self.engine = self._new_engine(max_batch, mh, mw, st)
        except Exception:
            # a failed growth (device out of memory for an oversized image / batch, rejected capacities) must not leave the
            # detector without a context: rebuild the previous one from the saved state, keep its capacity, re-raise
            self.engine = None
            if st is not None:
                self.engine = self._new_engine(*self._cap, st)
                if opt is not None:
                    self.load_optimizer_state(opt)
            raise
        self._cap = (max_batch, mh, mw)            # only once the new context is complete
        if opt is not None:
            self.load_optimizer_state(opt)

    def _new_engine(self, max_batch, mh, mw, st):
        eng = native.Engine(self._gpu, max_batch=max_batch, max_h=mh, max_w=mw, gaussian_sigma=params['gaussian_sigma'])
        try:
            if st is not None:
                eng.load_state(st)
            elif self._weights is not None:
                eng.set_weights(self._weights)
            if self._precision != 'f32':
                eng.set_option('precision', native.PRECISIONS[self._precision])
            self._apply_gradient_settings(eng)
            if self._gpu_branch_peaks:
                # the reference's own GPU branch of compute_peaks_from_heatmaps (:111-133): 17x17 un-normalised kernel, zero
                # padding, '>=' NMS -- NOT the golden CPU semantics; off by default
                eng.set_option('peaks_gpu_branch', 1)
        except Exception:
            eng.close()
            raise
        return eng

    # ---- gradient precision and the static loss scale (include/pose_mi355x.h: options "grad_precision", "loss_scale_log2") -----------------
    GRAD_PRECISIONS = {'f32': 0, 'f16': 2}

    @classmethod
    def _check_gradient_precision(cls, precision, loss_scale):
        """-> k with loss_scale == 2^k, k = 0 .. 24; ValueError for anything else and for an unknown precision"""
        if precision not in cls.GRAD_PRECISIONS:
            raise ValueError("gradient precision must be 'f32' or 'f16', got %r" % (precision,))
        try:
            m, e = math.frexp(float(loss_scale))
        except (TypeError, ValueError, OverflowError):
            m, e = 0.0, 0
        if m != 0.5 or not 0 <= e - 1 <= 24:
            raise ValueError('loss_scale must be a power of two in [1, 2^24], got %r' % (loss_scale,))
        return e - 1

    def set_gradient_precision(self, precision='f32', loss_scale=1.0):
        """How head_gradients, network_gradients, gradient_range and train_step compute the head's gradients.  precision 'f16': dw and dx of
        the 58 3x3 / 7x7 layers after conv4_2 with f16 operands and fp32 sums on the f16 matrix cores ('f32', the default: everything fp32);
        the trunk chain, the 1x1 layers, every db and Adam stay fp32 either way.  loss_scale, a power of two in [1, 2^24]: the loss gradients
        are multiplied by it on the device, so that gradients below the f16 range are not flushed (gradient_range shows what a scale leaves
        outside); it is taken out again exactly -- on the host in the arrays the *_gradients methods return, and in train_step through every
        layer's gradient scale, scale * 2^-k.  The setting stays with the detector: it is applied to every engine it creates and whenever
        training starts."""
        k = self._check_gradient_precision(precision, loss_scale)
        self._grad_precision, self._loss_scale_log2 = precision, k
        if self.engine is not None:
            self._apply_gradient_settings(self.engine)
            if self._train_on:
                self._fold_scales(self._trainable_layers())

    def _apply_gradient_settings(self, eng):
        eng.set_option('grad_precision', self.GRAD_PRECISIONS[self._grad_precision])
        eng.set_option('loss_scale_log2', self._loss_scale_log2)

    def _trainable_layers(self):
        """the layers with Adam state in the engine: the 82 after conv4_2, in mode 2 the ten trunk layers as well"""
        return (list(self.engine.TRUNK_LAYERS) if self._mode2 else []) + self.engine.head_layers()

    def _fold_scales(self, names):
        """the engine's gradient scale of each layer: the user's times 2^-k, which takes the loss scale out of the gradient in Adam's first
        line (exact: a power of two)"""
        unscale = 2.0 ** -self._loss_scale_log2
        for name in names:
            self.engine.train_set_grad_scale(name, self._grad_scales.get(name, 1.0) * unscale)

    def _unscale(self, arr):
        """the stored gradients are 2^k times the loss's, k that of the forward that made them: 2^-k times them, on the host (exact)"""
        k = self.engine.loss_grad_scale_log2()
        return arr if k == 0 else arr * np.float32(2.0 ** -k)

    # ---- host helpers with the reference's names and semantics -------------------------------------
    def compute_optimal_size(self, orig_img, img_size, stride=8):
        """Network input size (w, h) for an image: the SHORT side becomes `img_size`, the long side follows the aspect ratio
        (round-half-even, as np.round does) and is then rounded UP to a multiple of `stride`; a square image takes the second rule
        for its height.  Same results as reference pose_detector.py:57-73 (tests/test_oracle_vs_reference.py)."""
        h, w = orig_img.shape[:2]
        ratio = h / w                                        # the reference divides / multiplies by this float: keep its rounding

        def long_side(exact):
            return -(-int(np.round(exact)) // stride) * stride
        if h < w:
            return (long_side(img_size / ratio), int(img_size))
        return (int(img_size), long_side(img_size * ratio))

    def preprocess(self, img):
        """reference pose_detector.py:426-431 (host version, for `model=` callables; the built-in network
        fuses it into the first kernel)."""
        x_data = img.astype('f')
        x_data /= 255
        x_data -= 0.5
        x_data = x_data.transpose(2, 0, 1)[None]
        return x_data

    def _grow(self, batch, h, w):
        """Re-create the device context when an input exceeds its capacity (buffers are sized at creation)."""
        mb, mh, mw = self._cap
        if batch <= mb and h * w <= mh * mw:
            return
        self._make_engine(max(mb, batch), max(mh, h), max(mw, w))

    # ---- the hot path -----------------------------------------------------------------------------
    def __call__(self, orig_img):
        """reference pose_detector.py:484-517"""
        orig_img = np.asarray(orig_img)
        if self.precise:
            return self.detect_precise(orig_img)
        return self.detect_batch([orig_img])[0]

    def pad_image(self, img, stride, pad_value):
        """reference pose_detector.py:46-55: pad bottom / right to a multiple of `stride`."""
        h, w, _ = img.shape
        pad = [0] * 2
        pad[0] = (stride - (h % stride)) % stride  # down
        pad[1] = (stride - (w % stride)) % stride  # right
        img_padded = np.empty((h + pad[0], w + pad[1], 3), np.uint8)
        img_padded[...] = np.asarray(pad_value, dtype=np.uint8)
        img_padded[:h, :w, :] = img
        return img_padded, pad

    def detect_precise(self, orig_img):
        """reference pose_detector.py:433-482: average the network outputs over `inference_scales`, resized
        (cv2 INTER_CUBIC, restated in resize_cubic_*) to the ORIGINAL resolution, then the same post-process at that
        resolution with img_len = orig_img_w (:478) and no coordinate rescale.  The four forward passes and the
        full-resolution post-process run on the GPU.  With the native network the cubic resizes and the accumulation run on
        the device too (pmx_precise_*); with a plugged-in `model=` callable they are host code as in the reference."""
        orig_img = np.ascontiguousarray(orig_img, dtype=np.uint8)
        orig_img_h, orig_img_w, _ = orig_img.shape
        if self.model is None:
            return self._detect_precise_device(orig_img)
        pafs_sum = 0
        heatmaps_sum = 0
        for scale in params['inference_scales']:
            multiplier = scale * params['inference_img_size'] / min(orig_img.shape[:2])            # :442
            img = resize_cubic_u8(orig_img, math.ceil(orig_img_w * multiplier), math.ceil(orig_img_h * multiplier))
            padded_img, pad = self.pad_image(img, params['downscale'], (104, 117, 123))              # :445
            p_h, p_w = padded_img.shape[:2]
            h1s, h2s = self.model(self.preprocess(padded_img))
            paf = np.asarray(_data(h1s[-1]), dtype=np.float32)[0]
            heat = np.asarray(_data(h2s[-1]), dtype=np.float32)[0]
            tmp_paf = np.ascontiguousarray(paf.transpose(1, 2, 0))                                   # :453
            tmp_heatmap = np.ascontiguousarray(heat.transpose(1, 2, 0))                              # :454
            tmp_paf = resize_cubic_f32(tmp_paf, p_w, p_h)                                            # :461
            tmp_paf = tmp_paf[:p_h - pad[0], :p_w - pad[1], :]                                       # :462
            pafs_sum = pafs_sum + resize_cubic_f32(tmp_paf, orig_img_w, orig_img_h)                  # :463
            ds = params['downscale']
            tmp_heatmap = resize_cubic_f32(tmp_heatmap, tmp_heatmap.shape[1] * ds, tmp_heatmap.shape[0] * ds)   # :465
            tmp_heatmap = tmp_heatmap[:p_h - pad[0], :p_w - pad[1], :]                               # :466
            heatmaps_sum = heatmaps_sum + resize_cubic_f32(tmp_heatmap, orig_img_w, orig_img_h)      # :467
        n = len(params['inference_scales'])
        self.pafs = (pafs_sum / n).transpose(2, 0, 1)                                                # :469
        self.heatmaps = (heatmaps_sum / n).transpose(2, 0, 1)                                        # :470
        # post-process at the original resolution on the device (resize to the same size is the identity)
        self._grow(1, 8, 8)
        self.engine.set_maps(np.ascontiguousarray(self.pafs)[None], np.ascontiguousarray(self.heatmaps)[None])
        self.engine.postprocess(orig_img_h, orig_img_w, img_len=orig_img_w, scale_xy=None)           # :475-481
        self.all_peaks = self.engine.peaks(0)
        return unpack_results(self.engine.results())[0]

    def _detect_precise_device(self, orig_img, fetch_maps=True):
        """detect_precise with everything between the uint8 image and the result record on the device."""
        try:
            return self.detect_precise_batch([orig_img], fetch_maps=fetch_maps)[0]
        finally:                                    # (also when the reference's IndexError condition is raised: the maps and peaks exist)
            if fetch_maps and getattr(self, 'pafs', None) is not None and np.ndim(self.pafs) == 4:
                self.pafs, self.heatmaps = self.pafs[0], self.heatmaps[0]

    precise_images_per_call = 8       # images of different sizes per detect_precise call (sets the pixel budget the context grows to once)

    def precise_scaled_sizes(self, shape):
        """(h, w) of every inference scale of an image of `shape` in the reference's loop order (:441-443)."""
        sizes = []
        for scale in params['inference_scales']:
            multiplier = scale * params['inference_img_size'] / min(shape[:2])                     # :442
            sizes.append((math.ceil(shape[0] * multiplier), math.ceil(shape[1] * multiplier)))
        return sizes

    def detect_precise_batch(self, imgs, fetch_maps=False, return_exceptions=False):
        """`detect_precise` (reference pose_detector.py:433-482) for a list of uint8 BGR images -> list of (poses, scores), in the order given.
        The reference handles one image per call.  Images of ONE common size: every inference scale runs the n images as ONE batch through
        the network (a single 0.5x input is 23 x 31 feature maps -- too little for 256 CUs), the cubic resizes and the accumulation stay on
        the device per image, and the full-resolution post-process runs on the n averaged map sets at once.  Per image the result equals the
        single-image call up to the network's kernel-choice-by-launch-size rounding.  Images of DIFFERENT sizes
        (a data set): every (image, scale) pair is a segment of one network forward, as many images per call as the pixel budget allows
        (include/pose_mi355x.h::pmx_detect_precise_images); with fetch_maps, self.pafs / self.heatmaps are then lists of per-image arrays.
        Native network only (`model=` callables: loop).  Where the reference would raise for ONE image (IndexError, :197) the default
        raises as it does; `return_exceptions=True` puts the exception object into that image's slot and returns everybody else's result
        (a per-image loop over the reference loses nothing)."""
        if len(imgs) == 0:
            raise ValueError('detect_precise_batch needs at least one image')
        if self.model is not None:
            return [self.detect_precise(im) for im in imgs]
        if self._weights is None:
            raise RuntimeError('PoseDetector has no weights: pass weights_file=, weights= or model=')
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in imgs]
        for im in imgs:
            if im.ndim != 3 or im.shape[2] != 3:
                raise ValueError('detect_precise_batch needs uint8 H x W x 3 images')
        shape = imgs[0].shape
        if any(im.shape != shape for im in imgs):
            return self._detect_precise_mixed(imgs, fetch_maps, return_exceptions)
        orig_img_h, orig_img_w, _ = shape
        n = len(imgs)
        sizes = self.precise_scaled_sizes(shape)
        ds = params['downscale']
        big = max(sizes)
        self._grow(n, -(-big[0] // ds) * ds, -(-big[1] // ds) * ds)
        batch = np.stack(imgs)
        self.engine.precise_begin(orig_img_h, orig_img_w, n)
        # the largest scale is enqueued FIRST (its chain of launches is the critical path of the sequence) but keeps its position in the
        # reference's loop: the parts are summed in slot order (:463,467)
        order = sorted(range(len(sizes)), key=lambda i: -sizes[i][0] * sizes[i][1]) if self.precise_largest_first else range(len(sizes))
        for slot in order:
            self.engine.precise_add_scale(batch, sizes[slot][0], sizes[slot][1], slot=slot)          # :443-467
        self.engine.precise_finish()                                                                 # :469-470
        if fetch_maps:
            self.pafs, self.heatmaps = self.engine.get_maps()                                       # (n, 38 | 19, H, W)
        self.engine.postprocess(orig_img_h, orig_img_w, img_len=orig_img_w, scale_xy=None)           # :475-481
        rec = self.engine.results()
        self.all_peaks = self.engine.peaks(0) if n == 1 else None                                    # :475 (kept as the reference keeps it; a batch has no single set)
        return unpack_results(rec, return_exceptions=return_exceptions)

    def _detect_precise_mixed(self, imgs, fetch_maps, return_exceptions):
        """detect_precise_batch for images of different sizes: chunks within the context's pixel budget, each chunk one
        pmx_detect_precise_images call; results (and maps) in the caller's order."""
        ds = params['downscale']
        sizes = [self.precise_scaled_sizes(im.shape) for im in imgs]
        px = [sum((-(-h // ds) * ds) * (-(-w // ds) * ds) for h, w in sz) for sz in sizes]       # padded network-input pixels (:445)
        # grow ONCE: room for the precise_images_per_call largest images of the list (at least the largest one)
        per = max(1, min(len(imgs), int(self.precise_images_per_call)))
        want = sum(sorted(px, reverse=True)[:per])
        mb, mh, mw = self._cap
        if per > mb or want > mb * mh * mw:
            nb = max(mb, per)
            side = max(mh * mw, -(-want // nb))
            self._make_engine(nb, mh, -(-side // (mh * 8)) * 8)          # (max_w: a multiple of 8)
        mb, mh, mw = self._cap
        res = [None] * len(imgs)
        pafs, heats = [None] * len(imgs), [None] * len(imgs)
        for chunk in precise_chunks(px, mb * mh * mw, mb):
            self.engine.detect_precise_images([imgs[i] for i in chunk], [sizes[i] for i in chunk])   # :433-470 per image
            if fetch_maps:
                for k, i in enumerate(chunk):
                    pafs[i], heats[i] = self.engine.precise_image_maps(k)
            for k, r in enumerate(unpack_results(self.engine.results(), return_exceptions=True)):   # :475-481 per image
                res[chunk[k]] = r
        if fetch_maps:
            self.pafs, self.heatmaps = pafs, heats
        self.all_peaks = None                        # (several images: no single set, as for a same-size batch)
        if not return_exceptions:
            for r in res:                            # (the reference would have raised on that image's call)
                if isinstance(r, Exception):
                    raise r
        return res

    # ---- demo-chain helpers (reference pose_detector.py:267-424): host geometry that feeds the face / hand detectors -------
    _UNIT_BASE_LIMBS = (14, 3, 0, 13, 9)            # nose-neck, neck-left hip, neck-right hip, shoulder-ear (left, right)
    _UNIT_BASE_RATIO = (0.85, 2.2, 2.2, 0.85, 0.85)
    _UNIT_ALL_RATIO = (2.2, 1.7, 1.7, 2.2, 1.7, 1.7, 0.6, 0.93, 0.65, 0.85, 0.6, 0.93, 0.65, 0.85, 1, 0.2, 0.2, 0.25, 0.25)

    def compute_limbs_length(self, joints):
        """reference :267-277 -- per-limb length (0 where an endpoint is None) and the endpoint pairs."""
        pairs, lengths = [], np.zeros(len(params['limbs_point']))
        for i, (ja, jb) in enumerate(params['limbs_point']):
            a, b = joints[ja], joints[jb]
            if a is None or b is None:
                pairs.append(None)
                continue
            pairs.append([a, b])
            lengths[i] = np.linalg.norm(b[:-1] - a[:-1])
        return lengths, pairs

    def compute_unit_length(self, limbs_len):
        """reference :279-291 -- body 'unit length' from limb-length ratios; torso/head limbs are preferred."""
        base = limbs_len[list(self._UNIT_BASE_LIMBS)]
        known = base > 0
        if known.any():
            ratio = np.array(self._UNIT_BASE_RATIO)
            return np.sum(base[known] / ratio[known]) / np.count_nonzero(known)
        ratio = np.array(self._UNIT_ALL_RATIO)
        known = limbs_len > 0
        return np.sum(limbs_len[known] / ratio[known]) / np.count_nonzero(known)

    def get_unit_length(self, person_pose):
        """reference :293-297 (called by demo.py:32)"""
        return self.compute_unit_length(self.compute_limbs_length(person_pose)[0])

    # row j: how far (in unit lengths) the person's box extends above / below joint j when j is the top / bottom anchor,
    # and the preference of joint j as top / bottom anchor (smaller = preferred)   (reference :312-313, :342-343)
    _PERSON_TOP = ((0.9, 4), (1.9, 5), (1.9, 6), (2.9, 12), (3.7, 16), (1.9, 7), (2.9, 13), (3.7, 17), (4.0, 8), (5.5, 10), (7.0, 14),
                   (4.0, 9), (5.5, 11), (7.0, 15), (0.7, 2), (0.8, 3), (0.7, 0), (0.8, 1))
    _PERSON_BOTTOM = ((6.9, 9), (5.9, 6), (5.9, 7), (4.9, 14), (4.1, 16), (5.9, 8), (4.9, 15), (4.1, 17), (3.8, 4), (2.3, 2), (0.8, 0),
                      (3.8, 5), (2.3, 3), (0.8, 1), (7.1, 10), (7.0, 11), (7.1, 12), (7.0, 13))

    def crop_person(self, img, person_pose, unit_length):
        """reference :311-352: box around all visible joints -- 0.3 units to the sides, above / below by the padding of the
        preferred anchor joints.  One pass like the reference's, including its `elif` coupling: a joint that becomes the
        top anchor (or the new minimum) is not considered as bottom anchor (or maximum) in the same step."""
        top_i = bot_i = None                    # None = nothing chosen yet (the reference's sentinel of priority sys.maxsize)
        top_pos, left_pos = float('inf'), float('inf')
        bottom_pos, right_pos = 0, 0
        for i, joint in enumerate(person_pose):
            if not joint[2] > 0:
                continue
            if top_i is None or self._PERSON_TOP[i][1] < self._PERSON_TOP[top_i][1]:
                top_i = i
            elif bot_i is None or self._PERSON_BOTTOM[i][1] < self._PERSON_BOTTOM[bot_i][1]:
                bot_i = i
            if joint[1] < top_pos:
                top_pos = joint[1]
            elif joint[1] > bottom_pos:
                bottom_pos = joint[1]
            if joint[0] < left_pos:
                left_pos = joint[0]
            elif joint[0] > right_pos:
                right_pos = joint[0]
        if top_i is None or bot_i is None:      # the reference indexes its 18-entry padding tables with the sentinel 18
            raise IndexError('list index out of range')
        bbox = (int(left_pos - 0.3 * unit_length), int(top_pos - self._PERSON_TOP[top_i][0] * unit_length),
                int(right_pos + 0.3 * unit_length), int(bottom_pos + self._PERSON_BOTTOM[bot_i][0] * unit_length))
        return self.crop_image(img, bbox), bbox

    def crop_image(self, img, bbox):
        """reference :401-424 -- crop with zero padding where the box leaves the image."""
        left, top, right, bottom = bbox
        h, w, ch = img.shape
        out = np.zeros((bottom - top, right - left, ch), dtype=np.uint8)
        x0, y0, x1, y1 = max(0, left), max(0, top), min(w, right), min(h, bottom)
        if x1 > x0 and y1 > y0:
            out[y0 - top:y1 - top, x0 - left:x1 - left] = img[y0:y1, x0:x1]
        return out

    def crop_around_keypoint(self, img, keypoint, crop_size):
        """reference :299-309"""
        x, y = keypoint
        bbox = (int(x - crop_size), int(y - crop_size), int(x + crop_size), int(y + crop_size))
        return self.crop_image(img, bbox), bbox

    def crop_face(self, img, person_pose, unit_length):
        """reference :354-369 (demo.py:36): box around the nose, 1.2 units up, 0.8 down, 1 unit to each side."""
        nose = person_pose[JointType.Nose]
        if not nose[2] > 0:
            return None, None
        bbox = (int(nose[0] - unit_length), int(nose[1] - unit_length * 1.2),
                int(nose[0] + unit_length), int(nose[1] + unit_length * 0.8))
        return self.crop_image(img, bbox), bbox

    def crop_hands(self, img, person_pose, unit_length):
        """reference :371-399 (demo.py:44): a 0.95-unit box centred 30 % past the wrist along the forearm."""
        hands = {"left": None, "right": None}
        for side, wrist_j, elbow_j in (("left", JointType.LeftHand, JointType.LeftElbow),
                                       ("right", JointType.RightHand, JointType.RightElbow)):
            if person_pose[wrist_j][2] > 0:
                center = person_pose[wrist_j][:-1]          # a view, updated in place exactly as the reference does
                if person_pose[elbow_j][2] > 0:
                    center += (0.3 * (person_pose[wrist_j][:-1] - person_pose[elbow_j][:-1])).astype(center.dtype)
                hand_img, bbox = self.crop_around_keypoint(img, center, unit_length * 0.95)
                hands[side] = {"img": hand_img, "bbox": bbox}
        return hands

    def face_bbox(self, person_pose, unit_length):
        """The box crop_face cuts, without the pixels: (left, top, right, bottom) or None when the nose is not visible."""
        nose = person_pose[JointType.Nose]
        if not nose[2] > 0:
            return None
        return (int(nose[0] - unit_length), int(nose[1] - unit_length * 1.2),
                int(nose[0] + unit_length), int(nose[1] + unit_length * 0.8))

    def hand_bboxes(self, person_pose, unit_length):
        """The boxes crop_hands cuts, without the pixels: {"left": box | None, "right": box | None}.  Unlike crop_hands (and the
        reference) the pose is NOT modified: the moved wrist is a copy."""
        boxes = {"left": None, "right": None}
        for side, wrist_j, elbow_j in (("left", JointType.LeftHand, JointType.LeftElbow),
                                       ("right", JointType.RightHand, JointType.RightElbow)):
            if person_pose[wrist_j][2] > 0:
                center = np.array(person_pose[wrist_j][:-1], copy=True)
                if person_pose[elbow_j][2] > 0:
                    center += (0.3 * (person_pose[wrist_j][:-1] - person_pose[elbow_j][:-1])).astype(center.dtype)
                x, y = center
                crop_size = unit_length * 0.95
                boxes[side] = (int(x - crop_size), int(y - crop_size), int(x + crop_size), int(y + crop_size))
        return boxes

    def detect_batch(self, imgs):
        """Batched `__call__`: list of H x W x 3 uint8 BGR images -> list of (poses, scores), one per image in the order given (the
        reference handles one image per call).  Images of ONE common size run as a uniform batch; images of DIFFERENT sizes (the
        reference picks the network size per image, :490-493) run as a mixed batch -- one launch per layer over all size classes
        (include/pose_mi355x.h::pmx_detect_images) -- instead of one call per image.  Per image the result is what `__call__` returns
        for it, up to the kernel-choice-by-launch-size rounding of the network."""
        imgs = [np.asarray(im) for im in imgs]
        if len(imgs) == 0:
            raise ValueError('detect_batch needs at least one image')
        for im in imgs:
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise ValueError('detect_batch needs uint8 H x W x 3 images')
        shape = imgs[0].shape
        if any(im.shape != shape for im in imgs):
            return self._detect_mixed(imgs)
        orig_h, orig_w, _ = shape
        input_w, input_h = self.compute_optimal_size(imgs[0], params['inference_img_size'])   # :490
        map_w, map_h = self.compute_optimal_size(imgs[0], params['heatmap_size'])            # :491
        B = len(imgs)
        self._grow(B, input_h, input_w)
        batch = np.stack(imgs)
        scale = np.tile(np.array([orig_w / map_w, orig_h / map_h], dtype=np.float64), (B, 1))   # :513-514
        if self.model is None:
            if self.engine.weights_missing():
                raise RuntimeError('PoseDetector has no weights: pass weights_file=, weights= or model=')
            # cv2.resize (:493, identity when the size is unchanged) + preprocess + network + post-process, all on the GPU
            self.engine.forward_u8_resized(batch, input_h, input_w)                              # :493-499
            self.engine.postprocess(map_h, map_w, img_len=map_w, scale_xy=scale)                 # :501-516
        else:
            pafs, heats = [], []
            if (input_h, input_w) != (orig_h, orig_w):
                batch = self.engine.resize_u8(batch, input_h, input_w)                           # :493 on the device
            for im in batch:
                h1s, h2s = self.model(self.preprocess(im))                                      # :499
                pafs.append(np.asarray(_data(h1s[-1]), dtype=np.float32)[0])
                heats.append(np.asarray(_data(h2s[-1]), dtype=np.float32)[0])
            self.engine.set_maps(np.stack(pafs), np.stack(heats))
            self.engine.postprocess(map_h, map_w, img_len=map_w, scale_xy=scale)                # :501-516
        return unpack_results(self.engine.results())

    def _detect_mixed(self, imgs):
        """detect_batch for images of different sizes.  Images are sorted by network size (few segments), results return in the caller's
        order.  `model=` callables: one call per image, as the reference does."""
        if self.model is not None:
            return [self.detect_batch([im])[0] for im in imgs]
        if self._weights is None or self.engine.weights_missing():
            raise RuntimeError('PoseDetector has no weights: pass weights_file=, weights= or model=')
        net, mp = [], []
        for im in imgs:
            w_, h_ = self.compute_optimal_size(im, params['inference_img_size'])                 # :490
            mw_, mh_ = self.compute_optimal_size(im, params['heatmap_size'])                     # :491
            net.append((h_, w_))
            mp.append((mh_, mw_))
        order = sorted(range(len(imgs)), key=lambda i: (net[i], mp[i], i))
        px = sum(h * w for h, w in net)
        mb, mh, mw = self._cap
        if len(imgs) > mb or px > mb * mh * mw:
            # capacity is a pixel budget (max_batch x max_h x max_w) and an image count: grow both as needed
            nb = max(mb, len(imgs))
            side = max(mh * mw, -(-px // nb))
            self._make_engine(nb, mh, -(-side // (mh * 8)) * 8)          # (max_w: a multiple of 8)
        self.engine.detect_images([imgs[i] for i in order], [net[i] for i in order], [mp[i] for i in order])
        res = unpack_results(self.engine.results(), return_exceptions=True)
        out = [None] * len(imgs)
        for k, i in enumerate(order):
            out[i] = res[k]
        for r in out:                                  # (the reference would have raised on that image's call)
            if isinstance(r, Exception):
                raise r
        return out

    # ---- result images on the device (reference pose_detector.py:520-553, :574) ------------------------------------------------
    def draw_batch(self, imgs, poses_per_image, blend=False):
        """`[draw_person_pose(img, poses) for img, poses in zip(imgs, poses_per_image)]` in one launch on the device, byte for byte (an
        image without people comes back as an equal copy, where the host function returns the input object itself).  blend=True: each
        canvas as `demo.add_weighted(img, 0.6, canvas, 0.4, 0)`, the image every reference program saves.  Images of any sizes, host
        arrays or device tensors (native.Engine.render)."""
        return self.engine.render(imgs, poses_per_image, None, blend)

    # ---- validation loss (reference train_coco_pose_estimation.py:129-159, labels coco_data_loader.py:208-268) --------------------
    @staticmethod
    def _check_poses(poses, what='poses'):
        """-> (n, 18, 3) float64 rows (x, y, v); ValueError for another shape or a visible joint at a non-finite position"""
        try:
            p = np.asarray(poses, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError('%s: an (n, 18, 3) array of (x, y, v) rows expected' % what)
        if p.size == 0:
            return np.zeros((0, len(JointType), 3))
        if p.ndim != 3 or p.shape[1:] != (len(JointType), 3):
            raise ValueError('%s: an (n, 18, 3) array of (x, y, v) rows expected, got shape %r' % (what, p.shape))
        if not np.isfinite(p[..., :2][p[..., 2] > 0]).all():
            raise ValueError('%s: a visible joint (v > 0) at a non-finite position' % what)
        return p

    @staticmethod
    def _check_label_shape(shape_hw):
        try:
            h, w = (int(v) for v in shape_hw)
        except (TypeError, ValueError):
            raise ValueError('shape_hw: (h, w) expected, got %r' % (shape_hw,))
        if h < 8 or w < 8 or h % 8 or w % 8:
            raise ValueError('shape_hw: positive multiples of 8 expected (the network input size), got %d x %d' % (h, w))
        return h, w

    def generate_labels(self, shape_hw, poses):
        """The reference's label maps for one image of `shape_hw` = (h, w) network-input pixels (multiples of 8) and `poses` (n, 18, 3) rows
        (x, y, v): `generate_pafs` (params['paf_sigma']) and `generate_heatmaps` (params['heatmap_sigma']) of coco_data_loader.py:208-268,
        evaluated on the device -> (pafs (38, h, w), heatmaps (19, h, w)) float32."""
        h, w = self._check_label_shape(shape_hw)
        poses = self._check_poses(poses)
        self._grow(1, h, w)
        self.engine.loss_set_poses([poses], h, w, None, params['heatmap_sigma'], params['paf_sigma'])
        return self.engine.labels(0)

    @classmethod
    def _check_validation_args(cls, imgs, poses_per_image, ignore_masks):
        imgs = [np.asarray(im) for im in imgs]
        if len(imgs) == 0:
            raise ValueError('validation_loss needs at least one image')
        shape = imgs[0].shape
        for im in imgs:
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise ValueError('validation_loss needs uint8 H x W x 3 images')
            if im.shape != shape:
                raise ValueError('validation_loss needs images of one size (the validation loader yields insize x insize), got %r and %r'
                                 % (shape, im.shape))
        cls._check_label_shape(shape[:2])
        if len(poses_per_image) != len(imgs):
            raise ValueError('validation_loss: %d images but poses for %d' % (len(imgs), len(poses_per_image)))
        poses = [cls._check_poses(p, 'poses of image %d' % i) for i, p in enumerate(poses_per_image)]
        masks = None
        if ignore_masks is not None:
            if len(ignore_masks) != len(imgs):
                raise ValueError('validation_loss: %d images but %d ignore masks' % (len(imgs), len(ignore_masks)))
            masks = [np.asarray(m) for m in ignore_masks]
            for i, m in enumerate(masks):
                if m.shape != shape[:2]:
                    raise ValueError('ignore mask %d: shape %r, expected %r' % (i, m.shape, shape[:2]))
        return imgs, poses, masks

    def validation_loss(self, imgs, poses_per_image, ignore_masks=None):
        """What `Validator.evaluate` reports for one batch (train_coco_pose_estimation.py:146-157): the forward pass and compute_loss, the
        masked mean squared error of all six stages against the label maps of the poses -- on the device.  imgs: B uint8 BGR images of one
        size (multiples of 8; already at the network input size); poses_per_image: per image (n, 18, 3) rows (x, y, v) in those pixels;
        ignore_masks: per image an (h, w) array, non-zero = ignored (already dilated, coco_data_loader.py:340).  More images than the
        engine's batch run in chunks, averaged weighted by their sizes.  -> {'val/loss', 'val/paf', 'val/heat'} (floats) and
        'paf_stages', 'heat_stages' (six floats each).  Honours `precision=`."""
        imgs, poses, masks = self._check_validation_args(imgs, poses_per_image, ignore_masks)
        if self.model is not None:
            raise RuntimeError('validation_loss runs the built-in network: not available with a model= callable')
        if self.engine.weights_missing():
            raise RuntimeError('PoseDetector has no weights: pass weights_file=, weights= or model=')
        h, w = imgs[0].shape[:2]
        self._grow(1, h, w)
        mb = self._cap[0]
        total, paf, heat = 0.0, np.zeros(6), np.zeros(6)
        for i in range(0, len(imgs), mb):
            n = len(imgs[i:i + mb])
            self.engine.loss_set_poses(poses[i:i + n], h, w, None if masks is None else np.stack(masks[i:i + n]),
                                       params['heatmap_sigma'], params['paf_sigma'])
            t, p, q = self.engine.validate_batch(np.stack(imgs[i:i + n]))
            total += n * t
            paf += n * p
            heat += n * q
        total, paf, heat = total / len(imgs), paf / len(imgs), heat / len(imgs)
        return {'val/loss': float(total), 'val/paf': float(paf.sum()), 'val/heat': float(heat.sum()),
                'paf_stages': [float(v) for v in paf], 'heat_stages': [float(v) for v in heat]}

    def loss_gradients(self, imgs, poses_per_image, ignore_masks=None):
        """`validation_loss` plus where `loss.backward()` starts (train_coco_pose_estimation.py:90-126): the gradient of the total loss at
        the twelve stage outputs, on the device in the same forward.  Arguments as validation_loss.  -> its dictionary plus 'paf_grads' /
        'heat_grads': lists of six (B, 38 | 19, h/8, w/8) float32 arrays.  The gradient's scale 2 / N depends on the batch, so chunks
        cannot be merged: more images than the engine's batch raise ValueError.  The arrays are UN-SCALED: under a loss scale
        (set_gradient_precision) the device's values are multiplied by 2^-k on the host."""
        imgs, poses, masks = self._check_validation_args(imgs, poses_per_image, ignore_masks)
        if self.model is not None:
            raise RuntimeError('loss_gradients runs the built-in network: not available with a model= callable')
        if self.engine.weights_missing():
            raise RuntimeError('PoseDetector has no weights: pass weights_file=, weights= or model=')
        h, w = imgs[0].shape[:2]
        self._grow(1, h, w)
        if len(imgs) > self._cap[0]:
            raise ValueError('loss_gradients: %d images, the engine holds batches of %d (the gradients of chunks cannot be merged)'
                             % (len(imgs), self._cap[0]))
        self.engine.loss_set_poses(poses, h, w, None if masks is None else np.stack(masks), params['heatmap_sigma'], params['paf_sigma'])
        self.engine.loss_grad_enable(True)
        try:
            total, paf, heat = self.engine.validate_batch(np.stack(imgs))
            grads = [tuple(self._unscale(g) for g in self.engine.loss_grads(s)) for s in range(6)]
        finally:
            if not self._train_on:
                self.engine.loss_grad_enable(False)
        return {'val/loss': float(total), 'val/paf': float(paf.sum()), 'val/heat': float(heat.sum()),
                'paf_stages': [float(v) for v in paf], 'heat_stages': [float(v) for v in heat],
                'paf_grads': [g[0] for g in grads], 'heat_grads': [g[1] for g in grads]}

    def head_gradients(self, imgs, poses_per_image, ignore_masks=None):
        """`loss_gradients` plus the backward of the 82 layers after conv4_2 -- the layers the reference updates while conv1_1 .. conv4_2 are
        frozen (train_coco_pose_estimation.py:219-225) -- on the device.  Arguments as validation_loss.  -> loss_gradients' dictionary plus
        'grads': {layer name: (dW OIHW, db)} float32 and 'trunk_grad': (B, 512, h/8, w/8), the gradient at conv4_2's output.  More images
        than the engine's batch raise ValueError.  Computed as set_gradient_precision says; every array is UN-SCALED (the device's values
        times 2^-k on the host)."""
        imgs, poses, masks = self._check_validation_args(imgs, poses_per_image, ignore_masks)
        if self.model is not None:
            raise RuntimeError('head_gradients runs the built-in network: not available with a model= callable')
        if self.engine.weights_missing():
            raise RuntimeError('PoseDetector has no weights: pass weights_file=, weights= or model=')
        h, w = imgs[0].shape[:2]
        self._grow(1, h, w)
        if len(imgs) > self._cap[0]:
            raise ValueError('head_gradients: %d images, the engine holds batches of %d (the gradients of chunks cannot be merged)'
                             % (len(imgs), self._cap[0]))
        eng = self.engine
        eng.loss_set_poses(poses, h, w, None if masks is None else np.stack(masks), params['heatmap_sigma'], params['paf_sigma'])
        eng.loss_grad_enable(True)
        try:
            eng.backward_enable(True)
            total, paf, heat = eng.validate_batch(np.stack(imgs))
            eng.backward_head()
            grads = [tuple(self._unscale(g) for g in eng.loss_grads(s)) for s in range(6)]
            layer_grads = {name: tuple(self._unscale(g) for g in eng.layer_grad(name)) for name in eng.head_layers()}
            trunk = self._unscale(eng.trunk_grad())
        finally:
            if not self._train_on:          # (training lives on the backward's stores: they stay while it is on)
                eng.backward_enable(False)
                eng.loss_grad_enable(False)
        return {'val/loss': float(total), 'val/paf': float(paf.sum()), 'val/heat': float(heat.sum()),
                'paf_stages': [float(v) for v in paf], 'heat_stages': [float(v) for v in heat],
                'paf_grads': [g[0] for g in grads], 'heat_grads': [g[1] for g in grads], 'grads': layer_grads, 'trunk_grad': trunk}

    def network_gradients(self, imgs, poses_per_image, ignore_masks=None):
        """`head_gradients` continued through conv4_2 .. conv1_1: the gradients of all 92 layers, what the reference's loss.backward() gives
        once it has un-frozen the trunk (train_coco_pose_estimation.py:96-101, from iteration 2000 on).  Arguments and result as
        head_gradients, 'grads' with 92 entries.  The forward retains the trunk (engine mode 2), so its stem runs unfused.  More images than
        the engine's batch raise ValueError; not available while training is on (stop_training first).  The head as
        set_gradient_precision says, the trunk chain in fp32 from the head's (scaled) trunk gradient; every array is UN-SCALED (times 2^-k
        on the host)."""
        imgs, poses, masks = self._check_validation_args(imgs, poses_per_image, ignore_masks)
        if self.model is not None:
            raise RuntimeError('network_gradients runs the built-in network: not available with a model= callable')
        if self._train_on:
            raise RuntimeError('network_gradients switches retention on and off itself, training keeps it on: call stop_training() first')
        if self.engine.weights_missing():
            raise RuntimeError('PoseDetector has no weights: pass weights_file=, weights= or model=')
        h, w = imgs[0].shape[:2]
        self._grow(1, h, w)
        if len(imgs) > self._cap[0]:
            raise ValueError('network_gradients: %d images, the engine holds batches of %d (the gradients of chunks cannot be merged)'
                             % (len(imgs), self._cap[0]))
        eng = self.engine
        eng.loss_set_poses(poses, h, w, None if masks is None else np.stack(masks), params['heatmap_sigma'], params['paf_sigma'])
        eng.loss_grad_enable(True)
        try:
            eng.backward_enable(2)
            total, paf, heat = eng.validate_batch(np.stack(imgs))
            eng.backward_head()
            eng.backward_trunk()
            grads = [tuple(self._unscale(g) for g in eng.loss_grads(s)) for s in range(6)]
            layer_grads = {name: tuple(self._unscale(g) for g in eng.layer_grad(name)) for name in list(eng.TRUNK_LAYERS) + eng.head_layers()}
            trunk = self._unscale(eng.trunk_grad())
        finally:
            eng.backward_enable(False)
            eng.loss_grad_enable(False)
        return {'val/loss': float(total), 'val/paf': float(paf.sum()), 'val/heat': float(heat.sum()),
                'paf_stages': [float(v) for v in paf], 'heat_stages': [float(v) for v in heat],
                'paf_grads': [g[0] for g in grads], 'heat_grads': [g[1] for g in grads], 'grads': layer_grads, 'trunk_grad': trunk}

    def gradient_range(self, imgs, poses_per_image, ignore_masks=None):
        """Where the gradients of this batch fall in the f16 range at the current settings (set_gradient_precision): one retained forward
        and head backward, then per layer after conv4_2 the census of its masked gradient g as the f16 kernels would round it ->
        {layer: {'nonzero', 'flushed', 'subnormal', 'saturated', 'nan'}} (counts of elements: non-zero; non-zero but rounded to zero; f16
        subnormals; above 65504 in magnitude; NaN).  The data for choosing loss_scale: raise it while 'flushed' falls and 'saturated'
        stays 0.  Arguments as head_gradients."""
        imgs, poses, masks = self._check_validation_args(imgs, poses_per_image, ignore_masks)
        if self.model is not None:
            raise RuntimeError('gradient_range runs the built-in network: not available with a model= callable')
        if self.engine.weights_missing():
            raise RuntimeError('PoseDetector has no weights: pass weights_file=, weights= or model=')
        h, w = imgs[0].shape[:2]
        self._grow(1, h, w)
        if len(imgs) > self._cap[0]:
            raise ValueError('gradient_range: %d images, the engine holds batches of %d' % (len(imgs), self._cap[0]))
        eng = self.engine
        eng.loss_set_poses(poses, h, w, None if masks is None else np.stack(masks), params['heatmap_sigma'], params['paf_sigma'])
        eng.loss_grad_enable(True)
        try:
            eng.backward_enable(2 if self._train_on and self._mode2 else True)
            eng.validate_batch(np.stack(imgs))
            eng.backward_head()
            return {name: eng.g_census(name) for name in eng.head_layers()}
        finally:
            if not self._train_on:
                eng.backward_enable(False)
                eng.loss_grad_enable(False)

    # ---- training (reference train_coco_pose_estimation.py:204-235; head only as in its first 2000 iterations, or all 92 layers) -----------
    REFERENCE_GRAD_SCALES = {'conv4_3_CPM': 0.25, 'conv4_4_CPM': 0.25}      # GradientScaling (train_coco_pose_estimation.py:222-223)
    # ... and of the ten trunk layers (:213-217); in force once the trunk is trainable
    REFERENCE_TRUNK_GRAD_SCALES = dict.fromkeys(native.Engine.TRUNK_LAYERS, 0.25)

    def set_trainable(self, trunk=False):
        """Which layers train_step updates: the 82 layers after conv4_2 (default, the reference's first 2000 iterations) or, trunk=True, all 92
        (the reference from iteration 2000 on, enable_update on conv1_1 .. conv4_2).  The first trunk=True moves training to the engine's
        backward mode 2 (the forward retains the trunk, so its stem runs unfused); weights and Adam's state of the head carry over, the trunk
        joins with m = v = 0 and t = 0 and the reference's gradient scale 1/4 (REFERENCE_TRUNK_GRAD_SCALES).  trunk=False afterwards goes back
        to head-only steps and keeps the trunk's state in the stores, as Chainer's disable_update does."""
        trunk = bool(trunk)
        if trunk and not self._mode2:
            opt = self.optimizer_state() if self._train_on else None
            self.stop_training()
            self._mode2 = True
            scales = dict(self.REFERENCE_TRUNK_GRAD_SCALES, **self._grad_scales)
            if opt is not None:
                self.load_optimizer_state(opt)          # (a head-only state: it names the head's scales alone)
            self.set_optimizer(grad_scales=scales, **self._adam)
        self._trunk = trunk

    def _start_training(self):
        """Training mode of the current engine: loss gradients, retention and the optimiser's stores on (they stay on until stop_training)."""
        if self._train_on:
            return
        if self.model is not None:
            raise RuntimeError('training runs the built-in network: not available with a model= callable')
        if self._precision != 'f32':
            raise RuntimeError("training is fp32: create the detector with precision='f32'")
        if self.engine.weights_missing():
            raise RuntimeError('PoseDetector has no weights: pass weights_file=, weights= or model=')
        eng = self.engine
        eng.loss_grad_enable(True)
        try:
            eng.backward_enable(2 if self._mode2 else True)
            eng.train_enable(True)
            eng.train_set_adam(**self._adam)
            self._apply_gradient_settings(eng)
            # every trainable layer's scale carries 2^-k of the loss scale; a layer named without being trainable is the engine's to refuse
            trainable = self._trainable_layers()
            self._fold_scales(trainable + sorted(set(self._grad_scales) - set(trainable)))
        except Exception:
            eng.backward_enable(False)
            eng.loss_grad_enable(False)
            raise
        self._train_on = True

    def stop_training(self):
        """Leave training mode: frees the optimiser's and the backward's stores (the weights stay as trained; Adam's state is dropped --
        optimizer_state() first to keep it)."""
        if self._train_on:
            self._train_on = False
            self.engine.backward_enable(False)
            self.engine.loss_grad_enable(False)

    def set_optimizer(self, alpha=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, grad_scales=None):
        """Adam's hyper-parameters from the next train_step on (defaults: Chainer's, which the reference uses; it lowers alpha at 100 000 and
        200 000 iterations) and the per-layer gradient scales {layer: scale} (default: the reference's 1/4 for conv4_3_CPM and
        conv4_4_CPM and, once set_trainable(trunk=True) was called, for the ten trunk layers; layers not named: 1).  Trunk layers may be
        named only then."""
        self._adam = dict(alpha=float(alpha), beta1=float(beta1), beta2=float(beta2), eps=float(eps))
        old = self._grad_scales
        default = dict(self.REFERENCE_GRAD_SCALES, **(self.REFERENCE_TRUNK_GRAD_SCALES if self._mode2 else {}))
        self._grad_scales = dict(default if grad_scales is None else grad_scales)
        if self._train_on:
            self.engine.train_set_adam(**self._adam)
            self._fold_scales(sorted(set(old) | set(self._grad_scales) | set(self._trainable_layers() if self._loss_scale_log2 else ())))

    def train_step(self, imgs, poses_per_image, ignore_masks=None):
        """One iteration of the reference's training loop: the forward with compute_loss, the backward and Adam with the gradient scales,
        all on the device -- no gradient and no weight crosses to the host.  By default conv1_1 .. conv4_2 are frozen and the 82 layers after
        conv4_2 are updated; after set_trainable(trunk=True) the backward continues through the trunk and all 92 layers are.
        Arguments as head_gradients (uniform uint8 images at the network-input size; prepare_samples(mode='train') makes them).  ->
        {'main/loss', 'main/paf', 'main/heat'} (floats) and 'paf_stages', 'heat_stages': validation_loss's numbers of this batch BEFORE the
        update, under the reference's training names.  More images than the engine's batch raise ValueError."""
        imgs, poses, masks = self._check_validation_args(imgs, poses_per_image, ignore_masks)
        h, w = imgs[0].shape[:2]
        if self.model is None and self.engine.weights_missing():
            raise RuntimeError('PoseDetector has no weights: pass weights_file=, weights= or model=')
        self._grow(1, h, w)
        if len(imgs) > self._cap[0]:
            raise ValueError('train_step: %d images, the engine holds batches of %d (the gradients of chunks cannot be merged)'
                             % (len(imgs), self._cap[0]))
        self._start_training()
        eng = self.engine
        eng.loss_set_poses(poses, h, w, None if masks is None else np.stack(masks), params['heatmap_sigma'], params['paf_sigma'])
        eng.loss_enable(True)
        try:
            eng.forward_u8(np.stack(imgs))
            eng.backward_head()
            if self._trunk:
                eng.backward_trunk()
                eng.train_step()
            else:
                eng.train_step_head()
            paf, heat, _ = eng.loss_get()          # (the one synchronisation: the whole iteration is enqueued by now)
        finally:
            eng.loss_enable(False)
        return {'main/loss': float(paf.sum() + heat.sum()), 'main/paf': float(paf.sum()), 'main/heat': float(heat.sum()),
                'paf_stages': [float(v) for v in paf], 'heat_stages': [float(v) for v in heat]}

    def get_weights(self):
        """{layer name: (W OIHW, b)} float32 of all 92 layers as they are on the device now -- what weights.save_npz takes."""
        if self.model is not None:
            raise RuntimeError('get_weights reads the built-in engine: not available with a model= callable')
        return self.engine.get_weights()

    def optimizer_state(self):
        """Adam's state as a flat dictionary of NumPy arrays (np.savez takes it): 'adam' = (alpha, beta1, beta2, eps), and per head layer
        '<name>/m_W', '/v_W', '/m_b', '/v_b', '/t', '/scale' -- once the trunk was made trainable per layer of all 92.  With the weights
        (get_weights) it is what the reference's --resume restores."""
        self._start_training()
        out = {'adam': np.array([self._adam[k] for k in ('alpha', 'beta1', 'beta2', 'eps')], np.float64)}
        for name in (list(self.engine.TRUNK_LAYERS) if self._mode2 else []) + self.engine.head_layers():
            m_w, v_w, m_b, v_b, t = self.engine.train_get_state(name)
            out.update({name + '/m_W': m_w, name + '/v_W': v_w, name + '/m_b': m_b, name + '/v_b': v_b, name + '/t': np.array(t, np.int64),
                        name + '/scale': np.array(self._grad_scales.get(name, 1.0), np.float64)})
        return out

    def load_optimizer_state(self, state):
        """Install what optimizer_state() returned (or np.load of its np.savez) in this detector: training continues where it stopped.  A
        state that covers the trunk layers makes the trunk trainable in a detector that trained the head alone."""
        a = np.asarray(state['adam'], np.float64)
        names = sorted(k[:-len('/t')] for k in state.keys() if k.endswith('/t'))
        if not self._mode2 and any(n in self.engine.TRUNK_LAYERS for n in names):
            self.stop_training()
            self._mode2 = self._trunk = True
        self.set_optimizer(*[float(x) for x in a], grad_scales={n: float(state[n + '/scale']) for n in names if float(state[n + '/scale']) != 1.0})
        self._start_training()
        for n in names:
            self.engine.train_set_state(n, state[n + '/m_W'], state[n + '/v_W'], state[n + '/m_b'], state[n + '/v_b'], int(state[n + '/t']))

    # ---- sample preparation (reference coco_data_loader.py:61-205, 334-341) ----------------------------------------------------------
    @staticmethod
    def _check_sample_args(imgs, poses_per_image, ignore_masks, insize, mode, records):
        from . import samples as S
        # all-device input (contiguous uint8 torch tensors on the GPU; native.Engine.samples_prepare checks the rest) stays where it is
        given = list(imgs) + [m for m in (ignore_masks or []) if m is not None]
        dev = [hasattr(a, 'data_ptr') for a in given]
        if any(dev) != all(dev):
            raise ValueError('prepare_samples: the images and masks of one call are all host arrays or all device tensors')
        on_device = bool(dev) and dev[0]
        for a in (given if on_device else []):
            if str(a.dtype) != 'torch.uint8' or not a.is_cuda or not a.is_contiguous():
                raise ValueError('prepare_samples: a device image or mask is a contiguous uint8 tensor on the GPU')
        as_array = (lambda a: a) if on_device else np.asarray
        is_u8 = (lambda a: True) if on_device else (lambda a: a.dtype == np.uint8)
        imgs = [as_array(im) for im in imgs]
        if len(imgs) == 0:
            raise ValueError('prepare_samples needs at least one image')
        if mode not in ('val', 'train'):
            raise ValueError("prepare_samples: mode must be 'val' or 'train'")
        try:
            insize = int(insize)
        except (TypeError, ValueError):
            raise ValueError('prepare_samples: insize %r' % (insize,))
        if insize < 8 or insize % 8:
            raise ValueError('prepare_samples: insize must be a positive multiple of 8, got %d' % insize)
        for im in imgs:
            if not is_u8(im) or len(im.shape) != 3 or im.shape[2] != 3 or min(im.shape[:2]) < 1:
                raise ValueError('prepare_samples needs uint8 H x W x 3 images')
        if len(poses_per_image) != len(imgs):
            raise ValueError('prepare_samples: %d images but poses for %d' % (len(imgs), len(poses_per_image)))
        poses = [S.check_int_poses(np.zeros((0, len(JointType), 3), np.int32) if np.size(p) == 0 else p, 'poses of image %d' % i)
                 for i, p in enumerate(poses_per_image)]
        masks = None
        if ignore_masks is not None:
            if len(ignore_masks) != len(imgs):
                raise ValueError('prepare_samples: %d images but %d ignore masks' % (len(imgs), len(ignore_masks)))
            masks = [None if m is None else as_array(m) for m in ignore_masks]
            for i, m in enumerate(masks):
                if m is not None and tuple(m.shape) != tuple(imgs[i].shape[:2]):
                    raise ValueError('ignore mask %d: shape %r, expected %r' % (i, tuple(m.shape), tuple(imgs[i].shape[:2])))
        if records is not None:
            if len(records) != len(imgs):
                raise ValueError('prepare_samples: %d images but %d records' % (len(imgs), len(records)))
            for i, r in enumerate(records):
                if not isinstance(r, S.SampleRecord):
                    raise ValueError('record %d is no SampleRecord' % i)
                r.check()
                if tuple(r.src_hw) != tuple(imgs[i].shape[:2]) or r.insize != insize:
                    raise ValueError('record %d is for a %r image at insize %d, the image is %r at %d'
                                     % (i, r.src_hw, r.insize, imgs[i].shape[:2], insize))
        return imgs, poses, masks, insize

    def _records_for(self, imgs, poses, insize, mode, records):
        from . import samples as S
        if records is not None:
            return list(records)
        if mode == 'val':
            return [S.SampleRecord.val(tuple(im.shape[:2]), insize) for im in imgs]
        return [S.draw_augmentation(tuple(im.shape[:2]), p, insize) for im, p in zip(imgs, poses)]

    def prepare_samples(self, imgs, poses_per_image, ignore_masks=None, insize=368, mode='val', records=None):
        """`CocoDataLoader.generate_labels` without the label maps (coco_data_loader.py:334-341): the pixels on the device, the poses on the
        host.  imgs: uint8 BGR images of any sizes; poses_per_image: per image (n, 18, 3) INTEGER rows (x, y, v) in that image's pixels (the
        reference keeps int32 poses); ignore_masks: per image an (h, w) array at the image's size (non-zero = ignored) or None.
        Images and masks may instead ALL be contiguous uint8 torch tensors on the engine's GPU (masks of 0 | 1, as ignore_masks(device=True)
        gives them): they are read where they are; a mix of host arrays and device tensors raises ValueError.
        mode 'val': the resize to insize x insize; mode 'train': the reference's augmentation, drawn from `random` / `np.random` in its
        order (samples.draw_augmentation) unless `records` (samples.SampleRecord per image) gives every step.
        -> (images (B, insize, insize, 3) uint8, list of int32 poses in the samples' pixels, dilated masks (B, insize, insize) bool)."""
        from . import samples as S
        imgs, poses, masks, insize = self._check_sample_args(imgs, poses_per_image, ignore_masks, insize, mode, records)
        if self.model is not None:
            raise RuntimeError('prepare_samples runs on the built-in engine: not available with a model= callable')
        recs = self._records_for(imgs, poses, insize, mode, records)
        self._grow(1, insize, insize)
        mb = self._cap[0]
        out_i, out_m = [], []
        for i in range(0, len(imgs), mb):
            self.engine.samples_prepare(imgs[i:i + mb], None if masks is None else masks[i:i + mb], recs[i:i + mb], insize)
            a, m = self.engine.samples_get()
            out_i.append(a)
            out_m.append(m)
        return np.concatenate(out_i), [S.transform_poses(p, r) for p, r in zip(poses, recs)], np.concatenate(out_m)

    def ignore_masks(self, annotations_per_image, sizes, device=False):
        """The ignore masks `gen_ignore_mask.py` writes as PNG files (gen_masks' mask_miss, :23-37), rasterised on the device in one launch
        for a batch of images: annotations_per_image: per image ALL its annotation dictionaries in file order (CocoKeypoints.annotations);
        sizes: (h, w) per image.  -> a list of (h, w) bool arrays, or with device=True of uint8 tensors (0 | 1) on the engine's GPU that
        prepare_samples takes as they are.  Malformed segmentations raise ValueError (coco.mask_parts)."""
        from . import coco
        if self.model is not None:
            raise RuntimeError('ignore_masks runs on the built-in engine: not available with a model= callable')
        if len(annotations_per_image) != len(sizes):
            raise ValueError('ignore_masks: annotations for %d images, %d sizes' % (len(annotations_per_image), len(sizes)))
        parts = [coco.mask_parts(anns, h, w) for anns, (h, w) in zip(annotations_per_image, sizes)]
        return self.engine.coco_masks(sizes, parts, device=device)[0]

    def evaluate_batch(self, imgs, annotations_per_image, precise=False):
        """Detection and COCOeval's per-image step (coco.evaluate_image) for a list of images: `detect_batch` (precise: `detect_precise_batch`),
        then the OKS matrices and the matching walks on the device, on the result records where the post-process left them -- no pose
        visits the host on the way to its evaluation.  annotations_per_image: per image ALL its annotation dictionaries in file order
        (or coco.ground_truths of them).  -> (results per image as coco.evaluate_image gives them, poses per image, scores per image); the
        last two are what coco.results takes.  Images of one size run as one batch, a list of several sizes as one batch per size.  An image
        with more than coco.EVAL_MAX_GT annotations is evaluated by the host contract."""
        from . import coco
        if self.model is not None:
            raise RuntimeError('evaluate_batch runs on the built-in engine: not available with a model= callable')
        imgs = [np.asarray(im) for im in imgs]
        if len(imgs) == 0 or len(annotations_per_image) != len(imgs):
            raise ValueError('evaluate_batch: %d images, annotations for %d' % (len(imgs), len(annotations_per_image)))
        gts = [coco.ground_truths(a) for a in annotations_per_image]
        none = coco.ground_truths([])
        groups = {}
        for i, im in enumerate(imgs):
            groups.setdefault(tuple(im.shape), []).append(i)
        ev, poses, scores = [None] * len(imgs), [None] * len(imgs), [None] * len(imgs)
        for idx in groups.values():
            sub = [imgs[i] for i in idx]
            res = self.detect_precise_batch(sub) if precise else self.detect_batch(sub)
            large = [len(gts[i]['area']) > coco.EVAL_MAX_GT for i in idx]
            got = self.engine.coco_eval([none if big else gts[i] for i, big in zip(idx, large)])
            for k, i in enumerate(idx):
                poses[i], scores[i] = res[k]
                ev[i] = coco.evaluate_image(coco.detections(*res[k]), gts[i]) if large[k] else got[k]
        return ev, poses, scores

    def validation_loss_raw(self, imgs, poses_per_image, ignore_masks=None, insize=368):
        """`validation_loss` for raw validation data: images of any sizes, integer poses in each image's pixels, ignore masks at each
        image's size.  The resize to insize x insize, the mask's resize and 16 x 16 dilation, the label maps, the forward and the loss all
        run on the device; only the poses (n x 18 x 3 numbers) are scaled on the host.  -> the dictionary of validation_loss."""
        from . import samples as S
        imgs, poses, masks, insize = self._check_sample_args(imgs, poses_per_image, ignore_masks, insize, 'val', None)
        if self.model is not None:
            raise RuntimeError('validation_loss_raw runs the built-in network: not available with a model= callable')
        if self.engine.weights_missing():
            raise RuntimeError('PoseDetector has no weights: pass weights_file=, weights= or model=')
        recs = self._records_for(imgs, poses, insize, 'val', None)
        self._grow(1, insize, insize)
        mb = self._cap[0]
        total, paf, heat = 0.0, np.zeros(6), np.zeros(6)
        for i in range(0, len(imgs), mb):
            n = len(imgs[i:i + mb])
            self.engine.samples_prepare(imgs[i:i + n], None if masks is None else masks[i:i + n], recs[i:i + n], insize)
            t, p, q = self.engine.validate_samples([S.transform_poses(a, r) for a, r in zip(poses[i:i + n], recs[i:i + n])])
            total += n * t
            paf += n * p
            heat += n * q
        total, paf, heat = total / len(imgs), paf / len(imgs), heat / len(imgs)
        return {'val/loss': float(total), 'val/paf': float(paf.sum()), 'val/heat': float(heat.sum()),
                'paf_stages': [float(v) for v in paf], 'heat_stages': [float(v) for v in heat]}

    def detect_maps(self, paf, heat, map_h, map_w, img_len=None, scale_xy=None):
        """Post-process only (pose_detector.py:501-517) on network outputs paf (B,38,h,w), heat (B,19,h,w)."""
        self.engine.set_maps(paf, heat)
        self.engine.postprocess(map_h, map_w, img_len=map_w if img_len is None else img_len, scale_xy=scale_xy)
        return unpack_results(self.engine.results())


def precise_chunks(pixels, budget, max_images):
    """Cut a list of images (their network-input pixels, all scales) into consecutive runs of at most `max_images` images whose pixels fit
    `budget`; an image larger than the budget alone is a run of its own (the library refuses it with a capacity error)."""
    chunks, cur, used = [], [], 0
    for i, p in enumerate(pixels):
        if cur and (used + p > budget or len(cur) >= max_images):
            chunks.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += p
    if cur:
        chunks.append(cur)
    return chunks


def _data(v):
    return getattr(v, 'data', v)      # chainer.Variable-like or plain array


def unpack_results(records, return_exceptions=False):
    """Device result records -> [(poses, scores)] with the reference's return shapes and error behaviour.
    `return_exceptions`: an image on which the reference would raise (IndexError, :197) gets the exception OBJECT in its list slot
    instead of aborting the whole batch -- the reference, called once per image, only ever fails that image."""
    out = []
    for r in records:
        st = int(r['status'])
        if st & native.IMG_TRIPLE_MATCH:
            # the reference fails with IndexError at pose_detector.py:197 when a third subset matches
            err = IndexError('list assignment index out of range')
            if not return_exceptions:
                raise err
            out.append(err)
            continue
        # (capacity bits never reach this point: the library grows its buffers and re-runs the post-process, the reference
        #  has no limits on peaks / candidates / subsets / people)
        n = int(r['n_people'])
        if int(r['n_peaks']) == 0:
            out.append((np.empty((0, len(JointType), 3)), np.empty(0)))      # :509-510
        elif n == 0:
            out.append((np.array([]), np.empty(0)))                          # :264 np.array([]) / :516
        else:
            out.append((r['poses'][:n].copy(), r['scores'][:n].copy()))
    return out


# ---- cv2.resize(..., interpolation=cv2.INTER_CUBIC) restated (used by detect_precise only) ---------------------------
def _cubic_taps(dst, src):
    """Source indices (4 taps, replicate border) and float32 coefficients of OpenCV's bicubic (A = -0.75):
    fx = float((dx + 0.5) * scale - 0.5), scale = 1 / (dst / src) in double; sx = floor(fx); taps sx-1 .. sx+2."""
    scale = 1.0 / (float(dst) / float(src))
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    x = (f - s.astype(np.float32)).astype(np.float32)
    A = np.float32(-0.75)
    one = np.float32(1.0)
    c0 = ((A * (x + one) - np.float32(5) * A) * (x + one) + np.float32(8) * A) * (x + one) - np.float32(4) * A
    c1 = ((A + np.float32(2)) * x - (A + np.float32(3))) * x * x + one
    c2 = ((A + np.float32(2)) * (one - x) - (A + np.float32(3))) * (one - x) * (one - x) + one
    c3 = one - c0 - c1 - c2
    idx = np.stack([np.clip(s + k, 0, src - 1) for k in (-1, 0, 1, 2)])
    return idx, np.stack([c0, c1, c2, c3]).astype(np.float32)


def resize_cubic_f32(img, dst_w, dst_h):
    """`cv2.resize(float32 H x W x C, (dst_w, dst_h), interpolation=cv2.INTER_CUBIC)` restated (pose_detector.py:461-467):
    horizontal 4-tap pass then vertical 4-tap pass, float32 products summed left to right.  PARITY UNPINNED: OpenCV is
    not installable here (its SIMD paths may fuse multiply-adds)."""
    img = np.ascontiguousarray(img, dtype=np.float32)
    src_h, src_w = img.shape[:2]
    if (src_w, src_h) == (dst_w, dst_h):
        return img.copy()
    ix, cx = _cubic_taps(dst_w, src_w)
    iy, cy = _cubic_taps(dst_h, src_h)
    rows = img[:, ix[0]] * cx[0][None, :, None]
    for k in (1, 2, 3):
        rows = rows + img[:, ix[k]] * cx[k][None, :, None]
    out = rows[iy[0]] * cy[0][:, None, None]
    for k in (1, 2, 3):
        out = out + rows[iy[k]] * cy[k][:, None, None]
    return out


def resize_cubic_u8(img, dst_w, dst_h):
    """`cv2.resize(uint8 image, (dst_w, dst_h), interpolation=cv2.INTER_CUBIC)` restated (pose_detector.py:443): OpenCV's
    fixed-point path -- coefficients `saturate_cast<short>(c * 2048)`, int32 horizontal pass, vertical pass
    `(sum + (1 << 21)) >> 22`, saturated to uint8.  PARITY UNPINNED (no cv2 to compare against)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    src_h, src_w = img.shape[:2]
    if (src_w, src_h) == (dst_w, dst_h):
        return img.copy()
    ix, cx = _cubic_taps(dst_w, src_w)
    iy, cy = _cubic_taps(dst_h, src_h)
    ax = np.clip(np.rint(cx * np.float32(2048)), -32768, 32767).astype(np.int64)
    ay = np.clip(np.rint(cy * np.float32(2048)), -32768, 32767).astype(np.int64)
    src = img.astype(np.int64)
    rows = sum(src[:, ix[k]] * ax[k][None, :, None] for k in range(4))
    out = sum(rows[iy[k]] * ay[k][:, None, None] for k in range(4))
    out = (out + (1 << 21)) >> 22
    return np.clip(out, 0, 255).astype(np.uint8)


# ---- visualisation + CLI (reference pose_detector.py:520-579).  The host functions below are the contract of the device form
# (PoseDetector.draw_batch, native.Engine.render: include/pose_mi355x.h::pmx_render) and its oracle in the tests ----------------------
LIMB_COLORS = [
    [0, 255, 0], [0, 255, 85], [0, 255, 170], [0, 255, 255], [0, 170, 255],
    [0, 85, 255], [255, 0, 0], [255, 85, 0], [255, 170, 0], [255, 255, 0],
    [255, 0, 85], [170, 255, 0], [85, 255, 0], [170, 0, 255], [0, 0, 255],
    [0, 0, 255], [255, 0, 255], [170, 0, 255], [255, 0, 170]]
JOINT_COLORS = [
    [255, 0, 0], [255, 85, 0], [255, 170, 0], [255, 255, 0], [170, 255, 0],
    [85, 255, 0], [0, 255, 0], [0, 255, 85], [0, 255, 170], [0, 255, 255],
    [0, 170, 255], [0, 85, 255], [0, 0, 255], [85, 0, 255], [170, 0, 255],
    [255, 0, 255], [255, 0, 170], [255, 0, 85]]


def _draw_line(canvas, p1, p2, color, thickness=2):
    """All pixels within thickness/2 of the segment p1-p2 (stands in for cv2.line; OpenCV's exact raster is unpinned)."""
    h, w = canvas.shape[:2]
    x1, y1, x2, y2 = float(p1[0]), float(p1[1]), float(p2[0]), float(p2[1])
    r = thickness / 2.0
    xa, xb = int(max(0, math.floor(min(x1, x2) - r))), int(min(w - 1, math.ceil(max(x1, x2) + r)))
    ya, yb = int(max(0, math.floor(min(y1, y2) - r))), int(min(h - 1, math.ceil(max(y1, y2) + r)))
    if xa > xb or ya > yb:
        return
    ys, xs = np.mgrid[ya:yb + 1, xa:xb + 1]
    dx, dy = x2 - x1, y2 - y1
    L2 = dx * dx + dy * dy
    t = np.clip(((xs - x1) * dx + (ys - y1) * dy) / L2, 0, 1) if L2 > 0 else np.zeros_like(xs, dtype=float)
    d2 = (xs - (x1 + t * dx)) ** 2 + (ys - (y1 + t * dy)) ** 2
    canvas[ya:yb + 1, xa:xb + 1][d2 <= r * r + 0.25] = color


def _draw_disc(canvas, c, radius, color):
    h, w = canvas.shape[:2]
    cx, cy = int(c[0]), int(c[1])
    xa, xb, ya, yb = max(0, cx - radius), min(w - 1, cx + radius), max(0, cy - radius), min(h - 1, cy + radius)
    if xa > xb or ya > yb:
        return
    ys, xs = np.mgrid[ya:yb + 1, xa:xb + 1]
    canvas[ya:yb + 1, xa:xb + 1][(xs - cx) ** 2 + (ys - cy) ** 2 <= radius * radius] = color


def draw_person_pose(orig_img, poses):
    """reference pose_detector.py:520-553: limbs (thickness 2, shoulder-ear limbs 9 and 13 skipped) then joints (discs
    of radius 3) on a copy of the BGR image."""
    if len(poses) == 0:
        return orig_img
    canvas = np.array(orig_img, copy=True)
    rounded = np.asarray(poses).round().astype('i')
    for pose in rounded:
        for i, (limb, color) in enumerate(zip(params['limbs_point'], LIMB_COLORS)):
            if i != 9 and i != 13:
                a, b = pose[int(limb[0])], pose[int(limb[1])]
                if a[2] != 0 and b[2] != 0:
                    _draw_line(canvas, a[:2], b[:2], color, 2)
    for pose in rounded:
        for (x, y, v), color in zip(pose, JOINT_COLORS):
            if v != 0:
                _draw_disc(canvas, (x, y), 3, color)
    return canvas


def imread_bgr(path):
    """cv2.imread equivalent for the CLI: 8-bit BGR, alpha dropped (pose_detector.py:571)."""
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(path).convert('RGB'))[:, :, ::-1])


def imwrite_bgr(path, img):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(path)


def parse_args(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description='Pose detector')
    parser.add_argument('arch', choices=['posenet'], default='posenet', help='Model architecture')
    parser.add_argument('weights', help='weights file path (Chainer NPZ)')
    parser.add_argument('--img', '-i', default=None, help='image file path')
    parser.add_argument('--gpu', '-g', type=int, default=-1, help='GPU ID (negative value selects GPU 0: there is no CPU path)')
    parser.add_argument('--precise', action='store_true', help='do precise inference')
    parser.add_argument('--out', '-o', default='result.png', help='output image path')
    parser.add_argument('--precision', choices=['f32', 'f16'], default='f32',
                        help='f32 (default) or f16: the opt-in f16 inference mode (faster, accuracy contract in INTEGRATION.md section 4)')
    parser.add_argument('--render', choices=['host', 'device'], default='host',
                        help='where the result image is drawn: host (default, NumPy) or device (one launch; the same bytes)')
    return parser.parse_args(argv)


def main(argv=None):
    """`python -m <package>.pose_detector posenet weights.npz --img X [--gpu N] [--precise] [--render device]` (reference :555-579)."""
    args = parse_args(argv)
    pose_detector = PoseDetector(args.arch, args.weights, device=args.gpu, precise=args.precise, precision=args.precision)
    img = imread_bgr(args.img)
    poses, _ = pose_detector(img)
    img = pose_detector.draw_batch([img], [poses])[0] if args.render == 'device' else draw_person_pose(img, poses)
    print('Saving result into %s...' % args.out)
    imwrite_bgr(args.out, img)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
