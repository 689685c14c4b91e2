"""TEST INFRASTRUCTURE -- CPU restatement of the validation loss (reference train_coco_pose_estimation.py:41-73 on the label maps of
coco_data_loader.py:208-268).  NOT product code; it lives beside f16_emulation.py because oracle/ is frozen.

  labels      <- generate_pafs / generate_heatmaps through their restatements oracle/fixtures.py::render_pafs / render_heatmaps
  targets     <- the F.resize_images calls of compute_loss (:57-60) through oracle/postprocess_ref.py::resize_images_ref
  stage_loss  <- one stage of compute_loss (:62-66): ignored elements take the output as target (difference 0), float32 differences, their
                 squares summed in float64 (the reference's F.mean_squared_error is a float32 dot product; the recorded values of
                 tests/golden/loss_ref.npz carry that rounding), divided by ALL elements

tools/record_loss_goldens.py recorded the reference's own results; tests/test_validation_loss_host.py pins this file against them.
"""
import numpy as np

from oracle import fixtures
from oracle.postprocess_ref import resize_images_ref

HEAT_SIGMA, PAF_WIDTH = 7, 8          # params['heatmap_sigma'], params['paf_sigma'] (reference entity.py:60-61)


def labels(shape, poses, sigma=HEAT_SIGMA, width=PAF_WIDTH):
    """-> (pafs (38, h, w), heatmaps (19, h, w)) float32 of one image"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 18, 3)
    return fixtures.render_pafs(tuple(shape), poses, width), fixtures.render_heatmaps(tuple(shape), poses, sigma)


def targets(paf, heat, mask=None):
    """full-resolution labels of one image (38 | 19, h, w) and its ignore mask (h, w) or None -> (paf_t, heat_t, mask_t) at h/8 x w/8"""
    h, w = paf.shape[1:]
    fh, fw = h // 8, w // 8
    mask_t = np.zeros((fh, fw), bool)
    if mask is not None:
        mask_t = resize_images_ref((np.asarray(mask) != 0).astype('f')[None], fh, fw)[0] > 0
    return resize_images_ref(paf, fh, fw), resize_images_ref(heat, fh, fw), mask_t


def stage_loss(y_paf, y_heat, t_paf, t_heat, mask):
    """(B, 38 | 19, fh, fw) float32 outputs and targets, mask (B, fh, fw) bool -> (paf_loss, heat_loss) float64"""
    out = []
    for y, t in ((y_paf, t_paf), (y_heat, t_heat)):
        d = np.asarray(y, np.float32) - np.asarray(t, np.float32)
        d[np.broadcast_to(np.asarray(mask, bool)[:, None], d.shape)] = 0
        out.append(float((d.astype(np.float64) ** 2).sum() / d.size))
    return tuple(out)
