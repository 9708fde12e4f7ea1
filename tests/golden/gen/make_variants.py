#!/usr/bin/env python3
"""Manufactures small .cool streams that exercise decoder features the reference ENCODER cannot produce in
this container (common randomness needs VGG weights for --tune=wasserstein; a finest latent coarser than the
picture with a bilinear / bicubic final resize is not reachable from its CLI presets).  The streams are written
with this repo's bitstream writer (cool_chic_amd.writer: architecture and trained weights grown from the
`rgb192` fixture); the expected outputs are then produced by the REFERENCE decoder:

    python tests/golden/gen/make_variants.py            # writes tests/golden/<name>.cool
    for n in cr192 bicubic190 bilinear190; do python tests/golden/gen/dump_reference.py tests/golden/$n.cool $n; done
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from conftest import load_golden  # noqa: E402
from cool_chic_amd import writer  # noqa: E402
from oracle import oracle_py  # noqa: E402


def main():
    bs, z, _ = load_golden("rgb192")
    hdr, _, _ = oracle_py.split_stream(bs)[1][0][1][0]
    donor = writer.parse_cc_header(hdr)
    ints = z["cc0.nn_ints"]
    lat = [z[f"cc0.latent{g}"] for g in range(donor.n_grids)]
    variants = {
        # noise planes next to the latent planes (coolchic.py:179-183)
        "cr192": dict(flag_common_randomness=1),
        # finest latent at 1/2 resolution: bicubic resize of the 63 x 95 dense grid to 126 x 190, exactly x2 on both axes
        # (non-integer scales: bilinear190 below, and the derived pictures of tests/float_tail.py)
        "bicubic190": dict(img_size=(126, 190), latent_resolution=(1, 6), n_latent_grids=9, final_upsampling_type=2),
        # finest latent at 1/4 resolution, bilinear resize
        "bilinear190": dict(img_size=(126, 190), latent_resolution=(2, 6), n_latent_grids=8, final_upsampling_type=1),
    }
    for name, changes in variants.items():
        arch = writer.derive_arch(donor, **changes)
        nn = writer.encode_network(arch, writer.adapt_network(donor, ints, arch))
        stream = writer.encode_stream(writer.cc_header_bytes(arch), nn, writer.tile_latents(lat, donor, arch), bitdepth=8,
                                      frame_data_type=0)
        path = os.path.join(ROOT, "tests", "golden", name + ".cool")
        with open(path, "wb") as f:
            f.write(stream)
        print(name, len(stream), "bytes")


if __name__ == "__main__":
    main()
