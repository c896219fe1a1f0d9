"""The sparse tail's and halo's row tables in plain Python, restated from the comments of bayes-od-rc_amd/csrc/sparse_tables.h (not from
the kernel): which pixels each table computes, how they fall into runs, and how runs are cut into pieces and packed into tiles.
tests/test_sparse_tables_reference_host.py pins it to the header (tests/host/sparse_tables_dump.cpp runs the header's functions);
tests/test_gpu_sparse_masks.py replays the device's keep sets with it.

One image at a time.  `levels` is the list of (width, height) of the pyramid levels, `kept` one bool per pixel in dense order
(level, y, x).  Also here: the keep rule of post_sample_kernel for class weights whose kernel is zero (`predicted_pixel_masks`), which
lets a test choose how dense the keep set is, and the host search behind the hard-coded seeds of the GPU test's edge case.
"""
import numpy as np

ST_KEPT, ST_TAIL, ST_DIL, ST_HALO = 1, 2, 4, 8
EXT_ROWS = 320                      # extended rows a tile can stage (plan_tables.h XR_EXT_ROWS)
HALO_ROWS = 256                     # the halo's tile height; the tail's is 192 or 256

SQUARE_LEVELS = [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]                 # a 128x128 frame
ODD_LEVELS = [(25, 17), (13, 9), (7, 5), (4, 3), (2, 2)]                   # a 136x200 frame


def num_pixels(levels):
    return sum(w * h for w, h in levels)


def pixel_mask(anchor_index, levels, anchors_per_location=9):
    """bool [P]: the pixels with at least one kept anchor (pixel = anchor // anchors_per_location)."""
    mask = np.zeros(num_pixels(levels), bool)
    mask[np.asarray(anchor_index, np.int64) // anchors_per_location] = True
    return mask


def _level_views(levels, flat):
    """the flat per-pixel array as one [h, w] view per level"""
    views, p = [], 0
    for w, h in levels:
        views.append(flat[p:p + w * h].reshape(h, w))
        p += w * h
    return views


def _with_single_gaps(m):
    """m, plus every pixel that is not in m but whose left and right neighbours in its row both are"""
    out = m.copy()
    if m.shape[1] >= 3:
        out[:, 1:-1] |= m[:, :-2] & m[:, 2:]
    return out


def _dilated3x3(m):
    """the 3x3 dilation of m inside its level"""
    h, w = m.shape
    padded = np.zeros((h + 2, w + 2), bool)
    padded[1:-1, 1:-1] = m
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= padded[dy:dy + h, dx:dx + w]
    return out


def pixel_flags(levels, kept):
    """uint8 [P] of ST_* bits: kept; tail = kept or a single gap between two kept; dil = 3x3 dilation of the tail inside the level;
    halo = dil or a single gap between two dil."""
    kept = np.asarray(kept, bool)
    assert kept.shape == (num_pixels(levels),)
    tail, dil, halo = np.zeros_like(kept), np.zeros_like(kept), np.zeros_like(kept)
    for k, t, d, h in zip(*(_level_views(levels, a) for a in (kept, tail, dil, halo))):
        t[...] = _with_single_gaps(k)
        d[...] = _dilated3x3(t)
        h[...] = _with_single_gaps(d)
    return (kept * ST_KEPT + tail * ST_TAIL + dil * ST_DIL + halo * ST_HALO).astype(np.uint8)


def run_list(levels, member):
    """[(first pixel, pixels)]: the maximal runs of x-adjacent members, in pixel order.  A run never leaves its pyramid row."""
    runs, p0 = [], 0
    for m in _level_views(levels, np.asarray(member, bool)):
        h, w = m.shape
        for y in range(h):
            x = 0
            while x < w:
                if not m[y, x]:
                    x += 1
                    continue
                x1 = x
                while x1 < w and m[y, x1]:
                    x1 += 1
                runs.append((p0 + y * w + x, x1 - x))
                x = x1
        p0 += h * w
    return runs


def pack_runs(runs, n, rows):
    """Packs the runs, in order, into tiles of at most rows // n pixel slots and EXT_ROWS extended rows.  A piece of k pixels takes k
    slots and n * (k + 2) extended rows (k + 2 per sample); a run is cut where the open tile's slots or extended rows end; a tile
    closes when its slots are full, when not even a one-pixel piece fits its extended rows, or at the image's end.
    Returns (pieces, tiles): pieces = (first pixel, tile, first slot, first extended row, pixels),
    tiles = (first pixel, slots used, extended rows used, why it closed: "slots" | "ext" | "end")."""
    slots_max = rows // n
    assert slots_max >= 1 and EXT_ROWS // n >= 3
    pieces, tiles = [], []
    tile = None                                    # the open tile: first pixel, slots, extended rows
    for first, length in runs:
        p, left = first, length
        while left > 0:
            if tile is None:
                tile = [p, 0, 0]
            fits_ext = (EXT_ROWS - tile[2]) // n - 2        # the longest piece the free extended rows hold
            if fits_ext < 1:
                tiles.append((tile[0], tile[1], tile[2], "ext"))
                tile = None
                continue
            k = min(left, slots_max - tile[1], fits_ext)
            pieces.append((p, len(tiles), tile[1], tile[2], k))
            tile[1] += k
            tile[2] += n * (k + 2)
            p += k
            left -= k
            if tile[1] == slots_max:
                tiles.append((tile[0], tile[1], tile[2], "slots"))
                tile = None
    if tile is not None:
        tiles.append((tile[0], tile[1], tile[2], "end"))
    return pieces, tiles


def min_pixels_per_closed_tile(n, rows=256):
    """The fewest pixels of a tile that closed before the image's end: its slots were full (rows // n pixels), or fewer than 3n extended
    rows were free; k pixels cost at most 3n * k extended rows (one-pixel pieces), so more than (EXT_ROWS - 3n) / 3n pixels are in."""
    return max(1, min(rows // n, (EXT_ROWS - 3 * n) // (3 * n) + 1))


def tile_capacity(levels, n):
    """tiles one image's table can have at most: the engine sizes its buffers by this, per image"""
    return num_pixels(levels) // min_pixels_per_closed_tile(n) + 1


def table(levels, flags, bit, n, rows):
    runs = run_list(levels, (flags & bit) != 0)
    pieces, tiles = pack_runs(runs, n, rows)
    members = int(((flags & bit) != 0).sum())
    assert sum(k for *_, k in pieces) == members
    return {"runs": runs, "pieces": pieces, "tiles": tiles, "rows": rows,
            "summary": {"tiles": len(tiles), "valid_rows": n * members, "full_tiles": sum(1 for t in tiles if t[1] * n == rows)}}


def tables(levels, kept, n, tail_rows=192):
    """The flags and both tables of one image: {"flags", "tail", "halo"}."""
    flags = pixel_flags(levels, kept)
    return {"flags": flags, "tail": table(levels, flags, ST_TAIL, n, tail_rows), "halo": table(levels, flags, ST_HALO, n, HALO_ROWS)}


def filled_gaps(flags):
    """pixels the tail computes although they keep nothing"""
    return int((((flags & ST_TAIL) != 0) & ((flags & ST_KEPT) == 0)).sum())


# ------------------------------------------------------------------------------------------------
# Choosing the keep set through the class weights
# ------------------------------------------------------------------------------------------------
def lever_weights(weights, f, num_classes=8, anchors_per_location=9):
    """`weights` (synthetic.make_weights) with a class output layer that ignores its input: zero kernel, and a bias of f for class 0 of
    anchor type 0, 0 for every background class and -40 for every other class.  Every pixel of every image and sample then has the
    same class probabilities, only anchor type 0 can be kept, and post_sample_kernel's 30 categorical draws keep each pixel
    independently with one probability set by f."""
    w = dict(weights)
    layer = dict(w["pyramid_classification"])
    bias = np.full((anchors_per_location, num_classes), -40.0, np.float32)
    bias[:, -1] = 0.0
    bias[0, 0] = f
    layer["kernel"] = np.zeros_like(layer["kernel"])
    layer["bias"] = bias.reshape(-1)
    w["pyramid_classification"] = layer
    return w


def predicted_pixel_masks(f, seed, first_image_id, batch, levels, anchors_per_location=9, draws=30):
    """bool [batch, P]: the pixels lever_weights(f) keeps, by the host twin of the device's categorical uniforms.  A draw t = u * total
    picks class 0 if t < cdf[0] and the background otherwise (the other classes' probabilities vanish in float32); the anchor is kept
    iff class 0's count is not below the background's.  A prediction: the device's probabilities come out of its own softmax, so a
    draw on the CDF's edge may fall the other way there."""
    from oracle.philox import categorical_uniforms
    p = num_pixels(levels)
    p0 = np.float32(1.0) / (np.float32(1.0) + np.exp(np.float32(-f)))            # softmax of (f, -40 x 6, 0)
    masks = np.zeros((batch, p), bool)
    for b in range(batch):
        u = categorical_uniforms(seed, first_image_id + b, p * anchors_per_location, draws)[::anchors_per_location]
        fg = (u < p0).sum(axis=1)
        masks[b] = fg >= draws - fg
    return masks


def keep_probability(f, draws=30):
    """P[pixel kept] under lever_weights(f): at least half of `draws` Bernoulli(sigmoid(f)) draws are class 0"""
    from math import comb, exp
    q = 1.0 / (1.0 + exp(-f))
    return sum(comb(draws, k) * q ** k * (1 - q) ** (draws - k) for k in range((draws + 1) // 2, draws + 1))


def find_edge_calls(f, levels, batch=3, seeds=range(1, 1000), first_image_ids=(0, 7, 100), margin=2e-6):
    """The host search behind test_gpu_sparse_masks.py's EDGE_CALLS: (seed, first_image_id) pairs whose predicted masks give
      "nothing"  an image that keeps nothing beside images that keep something,
      "coarse"   an image whose only kept pixels lie in the two coarsest levels,
      "ends"     an image that keeps pixel 0 and an image that keeps pixel P - 1, in one call,
    one pair per property, the first found.  Pairs with a draw within `margin` of the CDF's edge at any pixel are passed over, so the
    device's rounding cannot turn the prediction.  Regenerate (a minute or two), from tests/ with the repository root on PYTHONPATH:
    python -c "import sparse_tables_reference as s; print(s.find_edge_calls(s.EDGE_F, s.ODD_LEVELS))" """
    from oracle.philox import categorical_uniforms
    p = num_pixels(levels)
    coarse0 = p - sum(w * h for w, h in levels[-2:])
    p0 = np.float32(1.0) / (np.float32(1.0) + np.exp(np.float32(-f)))
    found = {}
    for seed in seeds:
        for fid in first_image_ids:
            u = [categorical_uniforms(seed, fid + b, p * 9)[::9] for b in range(batch)]
            m = np.stack([2 * (x < p0).sum(axis=1) >= x.shape[1] for x in u])
            any_kept = m.any(axis=1)
            props = {"nothing": (~any_kept).any() and any_kept.any(),
                     "coarse": bool((any_kept & ~m[:, :coarse0].any(axis=1)).any()),
                     "ends": bool(m[:, 0].any() and m[:, p - 1].any())}
            news = [name for name, holds in props.items() if holds and name not in found]
            if not news or min(np.abs(x.astype(np.float64) - np.float64(p0)).min() for x in u) <= margin:
                continue
            assert np.array_equal(m, predicted_pixel_masks(f, seed, fid, batch, levels))
            for name in news:
                found[name] = (seed, fid)
            if len(found) == 3:
                return found
    return found


EDGE_F = -0.90625           # keeps about 1 % of the pixels (keep_probability); exact in bfloat16, as every f the GPU test uses
