"""torch restatement of full-network training for the tests: tests/train_ref.py::trajectory without the frozen stem -- all 92 layers are
leaves, conv1_1 .. conv4_2 are run (and differentiated) in every step -- with the same loss, the same autograd in a given dtype and the same
Adam of tests/adam_twin.py (float64: Chainer's formula; float32: the contract).  Every layer takes its first step at t = 1."""
import numpy as np

import adam_twin as A
from train_ref import TRUNK


def trajectory(weights, imgs, targets, steps, dtype, scales, n_stages=6, alpha=1e-4):
    """-> (the total loss before each of `steps` updates, the final {layer: [W, b]} of all 92 layers), everything in `dtype` ('float64' |
    'float32')"""
    import torch
    import torch.nn.functional as F
    td = getattr(torch, dtype)
    t_p, t_h, t_m = targets
    keep = torch.tensor(~t_m[:, None])
    tp, th = torch.tensor(t_p, dtype=td), torch.tensor(t_h, dtype=td)
    x = torch.tensor(imgs.transpose(0, 3, 1, 2).copy()).to(td) / 255 - 0.5
    names = list(weights)
    nd = np.dtype(dtype)
    P = {nm: [weights[nm][0].astype(nd), weights[nm][1].astype(nd)] for nm in names}
    M = {nm: [np.zeros_like(P[nm][0]), np.zeros_like(P[nm][1])] for nm in names}
    V = {nm: [np.zeros_like(P[nm][0]), np.zeros_like(P[nm][1])] for nm in names}
    step = A.step64 if dtype == 'float64' else A.step32
    losses = []
    for t in range(1, steps + 1):
        Q = {nm: [torch.tensor(a, requires_grad=True) for a in P[nm]] for nm in names}

        def c(nm, h, relu=True):
            h = F.conv2d(h, Q[nm][0], Q[nm][1], padding=Q[nm][0].shape[-1] // 2)
            return F.relu(h) if relu else h
        h = x
        for blk in (TRUNK[0:2], TRUNK[2:4], TRUNK[4:8]):
            for nm in blk:
                h = c(nm, h)
            h = F.max_pool2d(h, 2, 2)
        for nm in TRUNK[8:]:
            h = c(nm, h)
        feat = c('conv4_4_CPM', c('conv4_3_CPM', h))
        h1 = h2 = feat
        for i in range(1, 6):
            h1, h2 = c('conv5_%d_CPM_L1' % i, h1, i < 5), c('conv5_%d_CPM_L2' % i, h2, i < 5)
        loss = (((h1 - tp) * keep) ** 2).mean() + (((h2 - th) * keep) ** 2).mean()
        for s in range(2, n_stages + 1):
            h1 = h2 = torch.cat((h1, h2, feat), dim=1)
            for i in range(1, 8):
                h1, h2 = c('Mconv%d_stage%d_L1' % (i, s), h1, i < 7), c('Mconv%d_stage%d_L2' % (i, s), h2, i < 7)
            loss = loss + (((h1 - tp) * keep) ** 2).mean() + (((h2 - th) * keep) ** 2).mean()
        loss.backward()
        losses.append(float(loss.detach()))
        for nm in names:
            for j in (0, 1):
                if Q[nm][j].grad is None:
                    continue
                P[nm][j], M[nm][j], V[nm][j] = step(P[nm][j], M[nm][j], V[nm][j], Q[nm][j].grad.numpy(), scales.get(nm, 1.0), t, alpha=alpha)
    return np.array(losses), P
