#!/usr/bin/env python3
"""ARM-shape sweep (build container only): one small stream per (ARM inputs, hidden layers, IFCE yes / no) so that EVERY
instantiation of the pipelined entropy kernel - NV = ceil(inputs / 4) = 1..8, both variants - and its fall-back to the
generic kernel is reached by a test whose expected latents come from the REFERENCE decoder.

The reference ENCODER only trains the presets of cfg/dec (fixtures mop192 / vhop192 / vid3_*); the other shapes are written
with this repo's bitstream writer: architecture derived from the reference-encoded `rgb192` fixture, ARM / IFCE parameters
drawn (seeded) from the value distribution of its trained ones, its real latent pyramid (tiled to 32 x 320) as the symbols.  Each stream is then
decoded by the reference decoder (imported from /root/reference through ./shims) and the sha256 of every latent grid it
decoded is stored with the stream:

    python tests/golden/gen/make_arm_sweep.py          # writes tests/golden/arm_sweep.npz

Fixture = data: stream bytes (inputs) + reference-decoded hashes (expected outputs)."""
import hashlib
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from conftest import load_golden  # noqa: E402
from cool_chic_amd import writer  # noqa: E402
from cool_chic_amd._lib import lib  # noqa: E402
from oracle import oracle_py  # noqa: E402

# total ARM inputs (spatial contexts + IFCE features) the verdict of round 3 lists: NV = 1, 1, 2, 3, 4, 4, 5, 6, 7, 7, 8
DIMS = [3, 4, 8, 12, 14, 16, 20, 24, 26, 28, 32]
HIDDEN = [0, 1, 2, 3]
# shapes whose LDS footprint exceeds the pipelined kernel's: they must take the generic kernel, not fail
LARGE = [(29, 7, 0), (32, 7, 2), (31, 6, 2)]
IMG_SIZE = (32, 320)


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def configs():
    for dim in DIMS:
        for nh in HIDDEN:
            for n_ifce in (0, 2):
                if dim - n_ifce < 1:
                    continue
                yield dim, nh, n_ifce
    for c in LARGE:
        yield c


def build_stream(donor, donor_ints, latents, dim, n_hidden, n_ifce, seed):
    """Stream with `dim` ARM inputs (dim - n_ifce spatial contexts), `n_hidden` hidden layers, IFCE on every grid pair or off.
    The drawing rule lives in tests/arm_layouts.py, which the layout tests build their cases with as well."""
    import arm_layouts

    # 32 x 320: wavefront steps of up to 32 / 16 / 8 pixels on the three finest grids, i.e. the producers' 8-, 4- and 2-pixel tasks
    # all run (ccd_entropy_pipe.hip: n_max >= 25 / >= 9 / else), with 13.6 k symbols per stream
    stream, lat, _ = arm_layouts.build_stream(donor, donor_ints, latents, dim, n_hidden, n_ifce, seed, img_size=IMG_SIZE)
    return stream, lat


def reference_latents(stream: bytes):
    """The latent grids the REFERENCE decoder decodes from `stream` (hook on entropy_coding_latent_arm), finest first."""
    import tempfile

    import coolchic.bitstream.component.coolchic as bcc
    import coolchic.bitstream.decode as bdec

    got = []
    orig = bcc.entropy_coding_latent_arm

    def hook(enc, ctx, spatial_dim, *a, **kw):
        r = orig(enc, ctx, spatial_dim, *a, **kw)
        got.append(r.numpy().astype(np.int8).reshape(spatial_dim))
        return r

    bcc.entropy_coding_latent_arm = hook
    try:
        with tempfile.NamedTemporaryFile(suffix=".cool") as f:
            f.write(stream)
            f.flush()
            import contextlib
            import io

            with contextlib.redirect_stdout(io.StringIO()):
                frames = bdec.decode_video(f.name, None)
    finally:
        bcc.entropy_coding_latent_arm = orig
    img = (frames["0"].data[0] * 255.0).round().numpy().astype(np.uint8)
    return got[::-1], img  # decode order is coarsest first


def main():
    sys.path.insert(0, os.path.join(HERE, "shims"))
    sys.path.insert(1, "/root/reference")
    import torch

    torch.set_num_threads(1)
    bs, z, _ = load_golden("rgb192")
    hdr, _, _ = oracle_py.split_stream(bs)[1][0][1][0]
    donor = writer.parse_cc_header(hdr)
    ints = z["cc0.nn_ints"]
    lat = [z[f"cc0.latent{g}"] for g in range(donor.n_grids)]
    arrays, names = {}, []
    for i, (dim, nh, n_ifce) in enumerate(configs()):
        name = f"d{dim}_h{nh}_i{n_ifce}"
        stream, enc = build_stream(donor, ints, lat, dim, nh, n_ifce, seed=4000 + i)
        fh, ccs = oracle_py.split_stream(stream)[1][0]
        h_, nn_, l_ = ccs[0]
        cls = lib().ccd_network_kernel_class(h_, len(h_), nn_, len(nn_))
        ref, img = reference_latents(stream)
        assert len(ref) == len(enc)
        for a, b in zip(ref, enc):  # the reference decoder returns what was encoded
            assert np.array_equal(a, b), name
        arrays[name + ".stream"] = np.frombuffer(stream, dtype=np.uint8)
        arrays[name + ".latent_sha256"] = np.array([sha(g) for g in ref])
        arrays[name + ".planes_sha256_reference"] = np.array(sha(img))  # informative: float stages are 1-LSB noisy across builds
        names.append(name)
        print(name, len(stream), "bytes  class: pipe", cls & 1, "dyn", (cls >> 4) & 1, "NV", (cls >> 8) & 15, "layers", (cls >> 12) & 15)
    arrays["names"] = np.array(names)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "arm_sweep.npz"), **arrays)
    print(len(names), "streams")


if __name__ == "__main__":
    main()
