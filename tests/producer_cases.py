"""Inputs of tests/test_producer_late_path.py: picture sizes that reach every task size of the pipelined entropy kernel's
producers, latents crafted to reach every case of their window builder, and the oracle-side census of those cases.

Task size (ccd_entropy_pipe.hip, CCD_T8 = 25 / CCD_T4 = 9): 8 / 4 / 2 pixels for a grid whose longest wavefront step
n_max = min(H, (W - 1) / 10 + 1) is >= 25 / >= 9 / below.  A grid wider than 230 columns with H >= 25 whose longest step has >= 48
pixels, or ends in a task of 1..4 pixels, runs its body as one stream of pixels (StreamBody)."""
import numpy as np

K_MU_OFFSET, K_SCALE_OFFSET = 16384, 1280   # ccd_format.hpp: table index of mu = 0 / of log-scale 0 (b = 1)
AC_LO, AC_HI = -64, 63                      # the alphabet of the range coder

# (H, W) -> what the size is there for
SIZES = {
    (40, 260): "grid 0 on 8-pixel tasks (n_max 27), grid 1 (20 x 130) on 4-pixel tasks, grid 2 (10 x 65) on 2-pixel tasks",
    (48, 256): "streamed body with 25-26-pixel steps (the last task of a step has 1-2 pixels)",
    (56, 500): "streamed body with >= 48-pixel steps",
    (260, 40): "narrow and tall: steps of at most 4 pixels, 2-pixel tasks on every grid",
    (120, 100): "tall: steps of 10 pixels, grid 0 on 4-pixel tasks with no wider grid in front of it",
}


def task_pixels(h: int, w: int) -> int:
    """Pixels per producer task of an h x w grid coded in wavefront order (w > 9)."""
    n_max = min(h, (w - 1) // 10 + 1)
    return 8 if n_max >= 25 else (4 if n_max >= 9 else 2)


def crafted_latents(arch, seed: int = 20241018):
    """The same recipe on every grid: five bands along the longer side - Laplace noise (the common case), zeros (the ARM's
    smallest scales), a block of -64 and a block of +63 (mu at both ends of the alphabet: the window's top symbol clamps at
    both edges, and a window that reaches symbol 63 has the entry that runs to 2^24), and uniform noise over +-50 (scale
    indices above 1280: the 62-symbol windows)."""
    rng = np.random.default_rng(seed)
    out = []
    for g in range(arch.n_grids):
        h, w = arch.grid_h[g], arch.grid_w[g]
        a = np.clip(np.rint(rng.laplace(0.0, 1.0, size=(h, w))), -20, 20).astype(np.int8)
        along_w = w >= h
        n = w if along_w else h
        cuts = [n * k // 5 for k in range(6)]
        wild = rng.integers(-50, 51, size=(h, w)).astype(np.int8)

        def band(k):
            return (slice(None), slice(cuts[k], cuts[k + 1])) if along_w else (slice(cuts[k], cuts[k + 1]), slice(None))

        a[band(1)] = 0
        a[band(2)] = AC_LO
        a[band(3)] = AC_HI
        a[band(4)] = wild[band(4)]
        out.append(a)
    return out


def window_cases(mu_scale_idx: np.ndarray) -> dict:
    """Census of the window builder's cases over one grid, from the oracle's table indices [n_pixels][2] (mu, scale).
    A pixel with scale index <= 1280 gets the 14-symbol window whose top symbol is round(mu) + 6 clamped to [-51, 63], any
    other pixel the 62-symbol window with top round(mu) + 30 clamped to [-3, 63]."""
    mu = mu_scale_idx[:, 0].astype(np.int64)
    sc = mu_scale_idx[:, 1].astype(np.int64)
    rounded = ((mu + 128) >> 8) - 64
    narrow = sc <= K_SCALE_OFFSET
    top = np.where(narrow, rounded + 6, rounded + 30)
    lo = np.where(narrow, AC_LO + 13, AC_LO + 61)
    return {
        "narrow": int(narrow.sum()),
        "wide": int((~narrow).sum()),
        "top_clamped_low": int((narrow & (top < lo)).sum()),
        "top_clamped_high": int((narrow & (top > AC_HI)).sum()),
        "reaches_63": int((narrow & (top >= AC_HI)).sum()),    # entry 1 is symbol 63: P runs to 2^24
        "wide_reaches_63": int((~narrow & (top >= AC_HI)).sum()),
        "min_scale": int(sc.min()),
        "scale_0": int((sc == 0).sum()),
    }


def wide_envelope_network(donor, ints):
    """synth.kodak24_wide_envelope's network (there built inside the function that also encodes its 24 pictures): the IFCE rows
    that produce the donor's LAST feature doubled, the ARM's first-layer and stabiliser column that reads it halved.  The
    feature's worst case leaves 16 bits, so the stream runs the kernel instantiation with the device check of the features.
    Returns (header bytes, network bytes, parsed header)."""
    from cool_chic_amd import writer

    lay = writer.network_layout(donor)
    g = np.split(np.asarray(ints, dtype=np.int64).copy(), np.cumsum(lay)[:-1])
    dim, n_if = donor.total_context_arm, donor.output_feature_ifce
    pos = 0
    for k, f in enumerate(x for x in donor.input_features_ifce[:donor.n_grids] if x > 0):
        g[2][pos + (n_if - 1) * f: pos + n_if * f] *= 2
        g[3][k * n_if + n_if - 1] *= 2
        pos += n_if * f
    first = g[0][:dim * dim].reshape(dim, dim)
    first[:, dim - 1] = np.round(first[:, dim - 1] / 2.0)
    if donor.linear_stabiliser_arm:
        stab = g[0][-2 * dim:].reshape(2, dim)
        stab[:, dim - 1] = np.round(stab[:, dim - 1] / 2.0)
    nn = writer.encode_network(donor, np.concatenate(g).astype(np.int32))  # also sets the payload size / padding in `donor`
    return writer.cc_header_bytes(donor), nn, donor
