"""torch restatement of head-only training for the tests: the network of tests/test_gpu_head_backward.py with conv1_1 .. conv4_2 frozen (their
output computed once), autograd of the six-stage loss in a given dtype, and the Adam of tests/adam_twin.py (float64: Chainer's formula;
float32: the contract)."""
import numpy as np

import adam_twin as A

TRUNK = ('conv1_1', 'conv1_2', 'conv2_1', 'conv2_2', 'conv3_1', 'conv3_2', 'conv3_3', 'conv3_4', 'conv4_1', 'conv4_2')


def trajectory(weights, imgs, targets, steps, dtype, scales, n_stages=6, alpha=1e-4):
    """-> (the total loss before each of `steps` updates, the final {head layer: (W, b)}), everything in `dtype` ('float64' | 'float32')"""
    import torch
    import torch.nn.functional as F
    td = getattr(torch, dtype)
    t_p, t_h, t_m = targets
    keep = torch.tensor(~t_m[:, None])
    tp, th = torch.tensor(t_p, dtype=td), torch.tensor(t_h, dtype=td)

    def conv(h, w, b, relu=True):
        h = F.conv2d(h, w, b, padding=w.shape[-1] // 2)
        return F.relu(h) if relu else h
    with torch.no_grad():
        h = torch.tensor(imgs.transpose(0, 3, 1, 2).copy()).to(td) / 255 - 0.5
        for blk in (TRUNK[0:2], TRUNK[2:4], TRUNK[4:8]):
            for nm in blk:
                h = conv(h, torch.tensor(weights[nm][0], dtype=td), torch.tensor(weights[nm][1], dtype=td))
            h = F.max_pool2d(h, 2, 2)
        for nm in TRUNK[8:]:
            h = conv(h, torch.tensor(weights[nm][0], dtype=td), torch.tensor(weights[nm][1], dtype=td))
        x42 = h
    head = [nm for nm in weights if nm not in TRUNK]
    nd = np.dtype(dtype)
    P = {nm: [weights[nm][0].astype(nd), weights[nm][1].astype(nd)] for nm in head}
    M = {nm: [np.zeros_like(P[nm][0]), np.zeros_like(P[nm][1])] for nm in head}
    V = {nm: [np.zeros_like(P[nm][0]), np.zeros_like(P[nm][1])] for nm in head}
    step = A.step64 if dtype == 'float64' else A.step32
    losses = []
    for t in range(1, steps + 1):
        Q = {nm: [torch.tensor(a, requires_grad=True) for a in P[nm]] for nm in head}
        c = lambda nm, h, relu=True: conv(h, Q[nm][0], Q[nm][1], relu)
        feat = c('conv4_4_CPM', c('conv4_3_CPM', x42))
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
        for nm in head:
            for j in (0, 1):
                if Q[nm][j].grad is None:
                    continue
                P[nm][j], M[nm][j], V[nm][j] = step(P[nm][j], M[nm][j], V[nm][j], Q[nm][j].grad.numpy(), scales.get(nm, 1.0), t, alpha=alpha)
    return np.array(losses), P
