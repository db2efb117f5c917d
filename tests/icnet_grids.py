"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

The split-K launches of ICNet's four trainers at one shape, from the oracle modules' own arithmetic
(``workgroups()`` and the tile constants their ``kappa()`` is written on), and the pixels of one tile of each launch: what the
grid tests assert their preconditions with, on the GPU and without one.

A shape is in the trainer's own units: head ``(n, h8, w8)``, fusion ``(n, h16, w16)``, cascade and high-resolution
``(n, h32, w32)``.  A launch is ``(name, tiles, G, cap, (map height, map width, tile height, tile width))``; the trainer's own
launches come first (``OWN`` of them), then those of the next-shallower trainer it runs, whose bits it must reproduce.
``k_icnet_highres_wgrad1`` strides 256-pixel chunks of the flat map: its tile is ``(N Ho Wo, 1, 256, 1)``.
"""
import numpy as np

import icnet_cascade_train_oracle as ico
import icnet_fusion_train_oracle as ifo
import icnet_head_train_oracle as iho
import icnet_highres_train_oracle as iho3

OWN = {"head": 1, "fusion": 1, "cascade": 1, "highres": 3}
HEAD_CAP = 1024  # icnet_head_train_oracle.workgroups' own literal


def _cdiv(a, b):
    return -(-a // b)


def launches(trainer, n, h, w, mw=0):
    if trainer == "head":
        tiles, g = iho.workgroups(h, w, mw)
        return [("k_icnet_head_grad", tiles, g, HEAD_CAP, (2 * h, 2 * w, iho.TILE, iho.TILE))]
    if trainer == "fusion":
        tiles, g = ifo.workgroups(n, h, w, mw)
        return [("k_icnet_fusion_wgrad<128>", tiles, g, ifo.MAX_WG, (2 * h, 2 * w, ifo.TILE_H, ifo.TILE_W))] + launches(
            "head", n, 2 * h, 2 * w, mw)
    if trainer == "cascade":
        tiles, g = ico.workgroups(n, h, w, mw)
        return [("k_icnet_fusion_wgrad<256>", tiles, g, ico.MAX_WG, (2 * h, 2 * w, ifo.TILE_H, ifo.TILE_W))] + launches(
            "fusion", n, 2 * h, 2 * w, mw)
    assert trainer == "highres", trainer
    out = []
    for layer, name in ((3, "k_icnet_highres_wgrad<64>"), (2, "k_icnet_highres_wgrad<32>")):
        ho, wo = (32 >> layer) * h, (32 >> layer) * w
        tiles = n * _cdiv(ho, iho3.WG_TILE[0]) * _cdiv(wo, iho3.WG_TILE[1])
        out.append((name, tiles, iho3.workgroups(tiles, mw), iho3.MAX_WG, (ho, wo) + iho3.WG_TILE))
    pixels = n * 16 * h * 16 * w
    chunks = _cdiv(pixels, iho3.W1_CHUNK)
    out.append(("k_icnet_highres_wgrad1", chunks, iho3.workgroups(chunks, mw), iho3.MAX_WG, (pixels, 1, iho3.W1_CHUNK, 1)))
    return out + launches("cascade", n, h, w, mw)


def ragged(launch):
    """the launch's last tile is partial in one spatial direction or both"""
    ho, wo, th, tw = launch[4]
    return ho % th != 0 or wo % tw != 0


def uneven(launch):
    """G >= 3 groups and some of them run one more round than the others"""
    _, tiles, g, _, _ = launch
    return g >= 3 and tiles % g != 0


def capped(launch):
    """the launch runs at its cap, the tiles no multiple of it"""
    _, tiles, g, cap, _ = launch
    return tiles > cap and g == cap and tiles % cap != 0


def coherent_inputs(trainer, n, h, w, k, c_in=3, seed=7):
    """the sign-coherent inputs of ``icnet_highres_train_oracle.case(seed, ..., coherent=True)`` as the features entry of each
    trainer takes them, fp32: dL/dsub12_sum has one sign everywhere and every input below it is non-negative, so that the bound
    stays within a small factor of |g| for the tensors next to it.
      highres  the case itself: (conv5_4_k1, conv3_1, uint8 frame, weights, stats, labels, mask)
      cascade  (conv5_4_k1, conv3_1, conv3_sub1, weights, stats, labels, mask): conv3_sub1 is the float64 forward's F3
      fusion   (sub24_sum, conv3_sub1, weights, stats, labels, mask): the forward's maps of the case at
               (ceil(h16 / 2), ceil(w16 / 2)), cut to h16 x w16 (a cut keeps the signs)
      head     (sub12_sum, packed head, labels, mask): |N(0, 0.7)| features, class 0 everywhere, a head whose class-0 column is
               positive and dominates, scaled so that the logits stay within +-1 of the zero bias"""
    if trainer == "head":
        rng = np.random.default_rng(seed)
        x = np.abs(rng.standard_normal((n, h, w, 128)) * 0.7).astype(np.float32)
        kern = rng.uniform(-0.05, 0.05, (128, k))
        kern[:, 0] = rng.uniform(0.5, 1.0, 128)
        kern /= np.abs(x.reshape(-1, 128).astype(np.float64) @ kern).max()
        head = np.concatenate([kern.reshape(-1), np.zeros(k)]).astype(np.float32)
        return x, head, np.zeros((n, 8 * h, 8 * w), np.uint8), (rng.uniform(size=(n, 8 * h, 8 * w)) > 0.25).astype(np.float32)
    if trainer == "highres":
        return iho3.case(seed, n, h, w, k, c_in, coherent=True)
    hh, ww = (h, w) if trainer == "cascade" else (_cdiv(h, 2), _cdiv(w, 2))
    c54, c31, u8, d, stats, labels, mask = iho3.case(seed, n, hh, ww, k, coherent=True)
    fwd = iho3.forward(c54, c31, iho3.unit(u8), iho3.pack(d), stats, k)
    if trainer == "cascade":
        return c54, c31, fwd[2].astype(np.float32), {nm: d[nm] for nm in ico.NAMES}, stats[iho3.STATS_OWN:], labels, mask
    assert trainer == "fusion", trainer
    cut = lambda a, f: np.ascontiguousarray(a[:, :f * h, :f * w])
    return (cut(fwd[3].astype(np.float32), 1), cut(fwd[2].astype(np.float32), 2), {nm: d[nm] for nm in ifo.NAMES},
            stats[iho3.STATS_OWN + 512:], cut(labels, 16), cut(mask, 16))


def tile_mask(launch, n, t):
    """float64 [n, Ho, Wo, 1]: 1 on the pixels of tile ``t`` as the kernels number them -- image ``t // per_image``, then
    row-major over the image's tiles (k_icnet_fusion_wgrad, k_icnet_highres_wgrad); chunk ``t`` of the flat map for
    k_icnet_highres_wgrad1 (the caller reshapes)"""
    ho, wo, th, tw = launch[4]
    if tw == 1 and wo == 1:
        m = np.zeros(ho)
        m[t * th:(t + 1) * th] = 1.0
        return m
    ty, tx = _cdiv(ho, th), _cdiv(wo, tw)
    img, rem = divmod(t, ty * tx)
    i0, j0 = (rem // tx) * th, (rem % tx) * tw
    m = np.zeros((n, ho, wo, 1))
    m[img, i0:i0 + th, j0:j0 + tw] = 1.0
    return m
