"""NumPy restatement of every weight pack of the library (csrc/pack_index.h defines them, csrc/pmx_packs.hip builds them): the channel
maps, the direct pack and padded bias, the pack of the layer whose forward is the data gradient, the Winograd pack, conv1_1's
fused-kernel pack, and the f16 and bf16x3 packs (uint16 bits).  Written in scatter / whole-array form, independently of the header's
one-value-per-index form; nobody's production code.  Every function returns flat arrays laid out as the device buffers are, pads
included (+0.0f, or `fill` for index arrays)."""
import numpy as np

CK = 16
G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], np.float64)


def cout_pad(cout):
    return 64 if cout <= 64 else -(-cout // 128) * 128


def concat_map():
    """concat-buffer channel -> the reference's input channel of the pose network's Mconv1_* (38 PAF, 19 heat, 128 feature), -1: a pad"""
    m = np.full(192, -1)
    m[0:128] = 57 + np.arange(128)
    m[128:128 + 38] = np.arange(38)
    m[168:168 + 19] = 38 + np.arange(19)
    return m


def cpm_map(C):
    """face / hand networks: [feature 128 | heat C | pad to 16] -> the reference's F.concat((heat C, feature 128))"""
    m = np.full(-(-(128 + C) // CK) * CK, -1)
    m[0:128] = C + np.arange(128)
    m[128:128 + C] = np.arange(C)
    return m


def channel_map(kind, cin):
    """packed input channel -> reference input channel (kind 0: identity, 1: the pose concat buffer, 2 + C: face / hand)"""
    if kind == 1:
        return concat_map()
    if kind >= 2:
        return cpm_map(kind - 2)
    return np.concatenate([np.arange(cin), np.full((-cin) % CK, -1)])


def pack_weights(w, cin_map, cout_pad, fill=-1):
    """(cout, cin, T) -> [tap][chunk][cout_pad][16] flat, `fill` at every position no weight goes to"""
    cout, cin, T = w.shape
    nch = len(cin_map) // CK
    wp = np.full((T, nch, cout_pad, CK), fill, w.dtype)
    for k, src in enumerate(cin_map):
        if src >= 0:
            wp[:, k // CK, :cout, k % CK] = w[:, src, :].T
    return wp.reshape(-1)


def direct_pack(W, b, kind):
    """OIHW weights and bias -> (direct pack, padded bias)"""
    cout, cin, ks, _ = W.shape
    cp = cout_pad(cout)
    bp = np.zeros(cp, np.float32)
    bp[:cout] = b
    return pack_weights(np.ascontiguousarray(W, np.float32).reshape(cout, cin, ks * ks), channel_map(kind, cin), cp, 0), bp


def transposed_weights(w, cmap, t_cout):
    """(cout, cin, T) -> (t_cout, cout, T): row k = the layer's packed input channel k, taps rotated by 180 degrees; pad rows `-1` / zero"""
    wt = np.full((t_cout, w.shape[0], w.shape[2]), -1 if w.dtype.kind == 'i' else 0, w.dtype)
    for k in range(t_cout):
        if cmap[k] >= 0:
            wt[k] = w[:, cmap[k], ::-1]
    return wt


def transposed_pack(W, kind, t_cin_pad=None):
    """the direct pack of the layer whose forward is the data gradient; its input g has cout channels padded to t_cin_pad (default: to 64
    at least and to a multiple of 16).  -> (pack, t_cout, t_cin_pad)"""
    cout, cin, ks, _ = W.shape
    cmap = channel_map(kind, cin)
    t_cout = len(cmap) if kind == 1 else cin
    if t_cin_pad is None:
        t_cin_pad = max(64, -(-cout // CK) * CK)
    gmap = np.concatenate([np.arange(cout), np.full(t_cin_pad - cout, -1)])
    wt = transposed_weights(np.ascontiguousarray(W, np.float32).reshape(cout, cin, ks * ks), cmap, t_cout)
    return pack_weights(wt, gmap, cout_pad(t_cout), 0), t_cout, t_cin_pad


def _ggt(t):
    """t (3, 3, ...) float64 -> G t G^T (4, 4, ...): rows first, each sum associated as (G0 a + G1 b) + G2 c"""
    gg = [[(G[i, 0] * t[0, kx] + G[i, 1] * t[1, kx]) + G[i, 2] * t[2, kx] for kx in range(3)] for i in range(4)]
    return [[(gg[i][0] * G[j, 0] + gg[i][1] * G[j, 1]) + gg[i][2] * G[j, 2] for j in range(4)] for i in range(4)]


def _g1(a, b, c):
    return [(G[f, 0] * a + G[f, 1] * b) + G[f, 2] * c for f in range(4)]


def wino_pack(wp, ks, nch16, cout_pad):
    """direct pack -> Winograd pack [plane][chunk of 32][cout_pad / 32][k8-step 4][32][8]: float64, rounded once to float32"""
    cin_pad = nch16 * CK
    g = wp.reshape(ks, ks, nch16, cout_pad, CK).transpose(0, 1, 3, 2, 4).reshape(ks, ks, cout_pad, cin_pad).astype(np.float64)
    planes = []
    with np.errstate(invalid='ignore'):          # (0 * inf of a weight that is infinite: a NaN, as on the device)
        for sy in range(ks // 3):
            for sx in range(ks // 3):
                u = _ggt(g[3 * sy:3 * sy + 3, 3 * sx:3 * sx + 3])
                planes += [u[i][j] for i in range(4) for j in range(4)]
        if ks == 7:
            for sub in range(2):
                planes += _g1(g[6, 3 * sub], g[6, 3 * sub + 1], g[6, 3 * sub + 2])
            for sub in range(2):
                planes += _g1(g[3 * sub, 6], g[3 * sub + 1, 6], g[3 * sub + 2, 6])
            planes.append(g[6, 6])
    u = np.stack(planes).astype(np.float32)                                   # (planes, cout_pad, cin_pad)
    u = u.reshape(len(planes), cout_pad // 32, 32, cin_pad // 32, 4, 8).transpose(0, 3, 1, 4, 2, 5)
    return np.ascontiguousarray(u).reshape(-1)


def conv1_pack(wp, cout_pad=64):
    """conv1_1's direct pack [tap 9][1 chunk][cout_pad][16] -> [channel half 2][k-pair 14][k of the pair 2][channel 32], k = tap * 3 +
    input channel, the 28th k zero"""
    w = wp.reshape(9, cout_pad, CK)[:, :64, :3].transpose(1, 0, 2).reshape(64, 27)            # [channel][k]
    out = np.zeros((2, 28, 32), np.float32)
    out[:, :27] = w.reshape(2, 32, 27).transpose(0, 2, 1)
    return out.reshape(-1)


def edge_values():
    """float32 values at which a rounding can go wrong: +-0, subnormals, 2^-25 (half the smallest f16 subnormal: a tie to zero) and its
    neighbours, ties of f16 (1 + 2^-11, 1 + 3 * 2^-11: the even neighbour below / above) and of bf16 (1 + 2^-8, 1 + 3 * 2^-8), the f16
    saturation edge (65504, the last float32 below 65520, 65520), 1e30, +-inf, a NaN"""
    t25 = np.float32(2.0 ** -25)
    v = [0.0, -0.0, 1e-40, -1e-45, np.nextafter(t25, np.float32(0)), t25, np.nextafter(t25, np.float32(1)), -t25,
         1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 3 * 2.0 ** -8),
         65504, np.nextafter(np.float32(65520), np.float32(0)), 65520, -65520, 1e30, -1e30, np.inf, -np.inf, np.nan]
    return np.array(v, np.float32)


def splice_edge_values(W):
    """a copy of the weights W (any shape) with edge_values() at evenly spread places -> (weights, their flat places)"""
    e = edge_values()
    at = (np.arange(len(e)) * (W.size // len(e)) + W.size // (2 * len(e))).astype(np.int64)
    out = np.array(W, np.float32)
    out.reshape(-1)[at] = e
    return out, at


def f16_pack(wp):
    """direct pack -> f16 pack (uint16 bits, the same layout): clipped to +-65504, then rounded to nearest even by numpy.float16; a NaN
    becomes the quiet f16 NaN of its sign"""
    wp = np.ascontiguousarray(wp, np.float32)
    sign = (wp.view(np.uint32) >> 16).astype(np.uint16) & np.uint16(0x8000)
    with np.errstate(invalid='ignore'):
        h = np.clip(wp, -65504, 65504).astype(np.float16).view(np.uint16)
    return np.where(np.isnan(wp), sign | np.uint16(0x7e00), h)


def _bf16_bits(x):
    """float32 -> bf16 bits (uint16): integer round-to-nearest-even on the uint32 view; a NaN keeps its upper half with the quiet bit set"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    return np.where((u & 0x7fffffff) > 0x7f800000, (u >> 16) | 0x40, r).astype(np.uint16)


def _bf16_float(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def bf16x3_pack(wp, T, nch, cout_pad):
    """direct pack -> bf16x3 pack [tap][chunk][plane hi|mid|lo][cout_pad][16] (uint16 bits): hi = bf16(x), mid = bf16(x - hi),
    lo = bf16((x - hi) - mid), the subtractions in float32"""
    x = np.ascontiguousarray(wp, np.float32).reshape(T * nch, cout_pad, CK)
    with np.errstate(invalid='ignore'):
        hi = _bf16_bits(x)
        r1 = x - _bf16_float(hi)
        mid = _bf16_bits(r1)
        lo = _bf16_bits(r1 - _bf16_float(mid))
    return np.stack([hi, mid, lo], axis=1).reshape(-1)


def layer_packs(W, b, kind, transposed=True):
    """every pack a pose-network layer can have, keyed as Engine.get_pack keys them ('wino' of conv1_1, the (64, 3, 3, 3) layer, is its
    fused-kernel pack)"""
    cout, cin, ks, _ = W.shape
    w, bp = direct_pack(W, b, kind)
    out = {'w': w, 'b': bp}
    cin_pad = len(channel_map(kind, cin))
    if (cout, cin, ks) == (64, 3, 3):
        out['wino'] = conv1_pack(w)
    elif ks > 1 and cin_pad % 32 == 0:
        out['wino'] = wino_pack(w, ks, cin_pad // CK, cout_pad(cout))
    if transposed:
        tw, t_cout, t_cin_pad = transposed_pack(W, kind)
        out['t_w'] = tw
        if ks > 1 and t_cin_pad % 32 == 0:
            out['t_wino'] = wino_pack(tw, ks, t_cin_pad // CK, cout_pad(t_cout))
    return out
