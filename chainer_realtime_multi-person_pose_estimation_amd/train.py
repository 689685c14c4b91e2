"""The schedule of the reference's training loop (train_coco_pose_estimation.py:85-126, Updater.update_core) around PoseDetector.train_step:
when the trunk is un-frozen and when Adam's alpha falls.  No data loader, no COCO reader and no snapshots: those stay the caller's."""


def alpha_at(i, alpha_steps=((100000, 1e-5), (200000, 1e-6)), alpha0=1e-4):
    """Adam's alpha of iteration i: alpha0 (train_coco_pose_estimation.py:210) until the first threshold, then the alpha of the last
    threshold that i has reached (:102-105)."""
    alpha = alpha0
    for at, a in sorted(alpha_steps):
        if i >= at:
            alpha = a
    return alpha


def train_loop(det, batches, iterations, start=0, unfreeze_at=2000, alpha_steps=((100000, 1e-5), (200000, 1e-6)), on_log=None):
    """Iterations start .. iterations - 1 of the reference's loop on `det` (a PoseDetector): `iterations` is the iteration count at which
    training stops, as the reference's --iteration, and `start` where a resumed run continues (0: a fresh one).  Before iteration i:
      - the trunk (conv1_1 .. conv4_2) is trainable iff i >= unfreeze_at.  The reference tests `iteration == 2000`, which a run resumed
        past 2000 from weights and optimizer_state alone would miss; `>=` gives the same result for an unresumed run;
      - alpha is 1e-4, then the alpha of the last threshold of `alpha_steps` that i has reached, evaluated on i as the reference does.
        It is installed with det.set_optimizer(alpha=...) whenever it differs from the iteration before (and before the first iteration),
        so the other hyper-parameters and the gradient scales are the reference's.
    `batches`: any iterable of (imgs, poses_per_image, ignore_masks) as det.train_step takes them; the loop ends early when it runs out.
    on_log(i, result), if given, is called after every iteration.  -> the list of train_step's results."""
    results = []
    alpha = None
    it = iter(batches)
    for i in range(int(start), int(iterations)):
        try:
            imgs, poses, masks = next(it)
        except StopIteration:
            break
        det.set_trainable(trunk=i >= unfreeze_at)
        a = alpha_at(i, alpha_steps)
        if a != alpha:
            det.set_optimizer(alpha=a)
            alpha = a
        results.append(det.train_step(imgs, poses, masks))
        if on_log is not None:
            on_log(i, results[-1])
    return results
