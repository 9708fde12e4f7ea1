"""Case builders of tests/test_inter_deltas.py: one P / B frame of a video fixture as the two candidates of ccd_dsens_add_inter,
and the brute force they are compared with.

The brute force never touches the new kernel or handle: a latent is moved on the host, the cool-chic goes through given-latent
slots of a DecodeBatch with its float output kept, ccd_inter_reconstruct joins it with the partner's base output and the references,
QualityMeter.score_planes gives the exact integer SSE, and the base SSE is subtracted.

Inputs.  The base latents are the fixture's own (random latents in the motion cool-chic give flows that mostly read the border);
in every grid the two corners are forced to -64 and 63 and a few positions to the alphabet's ends.  The source is the
reconstruction of a second latent set, base plus a seeded integers(-2, 3) on every grid of both cool-chics, so that the deltas
take both signs."""
import ctypes as C
import os

import numpy as np

from conftest import GOLDEN

SENTINEL = -2 ** 63
FDT_NAMES = ["rgb", "yuv420", "yuv444"]
ROLES = ("residue", "motion")


def parse_video(name):
    """[(frame header, [(arch with geometry, header bytes, nn, payload)] per cool-chic, display index, reference display
    indices)] in coding order, through the oracle's stream walker and the library's coding structure."""
    from cool_chic_amd import writer
    from cool_chic_amd.bitstream.header import VideoHeader
    from oracle import oracle_py

    with open(os.path.join(GOLDEN, name + ".cool"), "rb") as f:
        bs = f.read()
    _, frames = oracle_py.split_stream(bs)
    vh = VideoHeader()
    vh.read_header(bs)
    structure = vh.get_coding_structure()
    out = []
    for k, (fh, ccs) in enumerate(frames):
        out.append((fh, [(writer.parse_cc_header(hdr), hdr, nn, lat) for hdr, nn, lat in ccs], int(structure[k]["display_order"]),
                    [int(r) for r in structure[k]["index_references"]]))
    return out


_DECODED = {}


def decoded_planes(name):
    """{display index: three device planes} of the fixture as the library decodes it (the references of its inter frames)."""
    import torch

    from cool_chic_amd.bitstream.decode import decode_video
    from cool_chic_amd.bitstream.intercoding import _integer_planes

    if name not in _DECODED:
        frames = decode_video(os.path.join(GOLDEN, name + ".cool"))
        _DECODED[name] = {int(d): _integer_planes(fd, torch.device("cuda:0")) for d, fd in frames.items()}
    return _DECODED[name]


def sample_positions(h, w, rng, n_random=24):
    """tests/test_distortion_deltas.py::_sample_positions: four corners, four edge midpoints, n_random random positions."""
    pos = {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1)}
    want = min(h * w, len(pos) + n_random)
    while len(pos) < want:
        pos.add((int(rng.integers(h)), int(rng.integers(w))))
    return sorted(pos)


class _CoolChic:
    """One cool-chic of the frame: its architecture, two latent sets, and 64 given-latent slots (float output kept, no planes
    of their own - as the decoder adds the cool-chics of an inter frame) that read rows of one device buffer."""

    N = 64

    def __init__(self, arch, nn, base, seed):
        import torch

        from cool_chic_amd import DecodeBatch

        self.arch, self.nn = arch, nn
        self.n = int(arch.n_grids)
        self.hw = [(int(arch.grid_h[g]), int(arch.grid_w[g])) for g in range(self.n)]
        self.sizes = [h * w for h, w in self.hw]
        self.off = np.concatenate([[0], np.cumsum([(s + 255) // 256 * 256 for s in self.sizes])]).astype(np.int64)
        rng = np.random.default_rng(seed)
        self.lat = [a.copy() for a in base]
        for a in self.lat:  # the alphabet's ends: the two corners, and a few positions anywhere
            a.flat[0], a.flat[-1] = -64, 63
            where = rng.choice(a.size, size=min(a.size, 4), replace=False)
            a.flat[where] = rng.choice([-64, 63], size=len(where))
        self.lat2 = [np.clip(a.astype(np.int16) + rng.integers(-2, 3, size=a.shape), -64, 63).astype(np.int8) for a in self.lat]
        self.buf = torch.zeros((self.N, int(self.off[-1])), dtype=torch.int8, device="cuda")
        self.batch = DecodeBatch(0)
        for k in range(self.N):
            self.batch.add_latents_device(arch, nn, [self.buf[k].data_ptr() + int(self.off[g]) for g in range(self.n)], 0, 0, owner=self.buf)
        self.lat_dev = torch.from_numpy(self.flat(self.lat)).cuda()

    def flat(self, lat):
        row = np.zeros(int(self.off[-1]), np.int8)
        for g, a in enumerate(lat):
            row[self.off[g]:self.off[g] + a.size] = a.ravel()
        return row

    def ptrs(self, dev_row):
        return [dev_row.data_ptr() + int(self.off[g]) for g in range(self.n)]

    def outputs(self, lats):
        """Device float outputs [C][H][W] (valid until the next call) of up to 64 latent sets."""
        import torch

        assert len(lats) <= self.N
        host = np.stack([self.flat(l) for l in lats] + [self.flat(lats[0])] * (self.N - len(lats)))
        self.buf.copy_(torch.from_numpy(host))
        torch.cuda.synchronize()
        self.batch.run(); self.batch.wait()
        return [torch.as_tensor(self.batch.output_device(k), device="cuda")[0] for k in range(len(lats))]


class InterCase:
    """Frame `coding_index` of a video fixture.  `formats`: (frame_data_type index, bitdepth) replaces the frame's and takes
    seeded random reference planes; `warp_filter_size` replaces the header's (nothing else of the call changes)."""

    def __init__(self, name, coding_index, seed=0, formats=None, warp_filter_size=None):
        import torch

        from cool_chic_amd import DecodeBatch

        self.name = f"{name}[{coding_index}]"
        fh, ccs, _, ref_display = parse_video(name)[coding_index]
        assert fh.frame_type in (1, 2) and len(ccs) == 2
        self.frame_type = int(fh.frame_type)
        self.fdt, self.bd = (int(fh.frame_data_type), int(fh.bitdepth)) if formats is None else formats
        self.taps = int(fh.warp_filter_size) if warp_filter_size is None else int(warp_filter_size)
        self.gflow = [int(v) for v in fh.global_flow]
        self.H, self.W = int(ccs[0][0].img_size[0]), int(ccs[0][0].img_size[1])
        dt = torch.uint8 if self.bd == 8 else torch.uint16
        ch, cw = (self.H // 2, self.W // 2) if self.fdt == 1 else (self.H, self.W)
        self.shapes = [(self.H, self.W), (ch, cw), (ch, cw)]
        self.dtype = dt
        n_refs = 2 if self.frame_type == 2 else 1
        if formats is None:
            planes = decoded_planes(name)
            self.refs = [[p.clone() for p in planes[d]] for d in ref_display[:n_refs]]
        else:
            rng = np.random.default_rng([seed, 77])
            npdt = np.uint8 if self.bd == 8 else np.uint16
            self.refs = [[torch.from_numpy(rng.integers(0, 2 ** self.bd, size=s).astype(npdt)).cuda() for s in self.shapes]
                         for _ in range(n_refs)]
        # the fixture's own latents, decoded once
        dec = DecodeBatch(0)
        for arch, hdr, nn, lat in ccs:
            dec.add(hdr, nn, lat, 0, 0)
        dec.run(); dec.wait()
        self.cc = {}
        for i, role in enumerate(ROLES):
            arch, _, nn, _ = ccs[i]
            base = [dec.latent(i, g) for g in range(int(arch.n_grids))]
            self.cc[role] = _CoolChic(arch, nn, base, [seed, i, len(name)])
        dec.close()
        # base and second-set float outputs of both cool-chics (the partners), and the source
        self.out = {r: self.cc[r].outputs([self.cc[r].lat])[0].clone() for r in ROLES}
        self.out2 = {r: self.cc[r].outputs([self.cc[r].lat2])[0].clone() for r in ROLES}
        self.src = self.reconstruct(self.out2["residue"], self.out2["motion"])
        self.base_planes = self.reconstruct(self.out["residue"], self.out["motion"])
        self._maps = {}

    def new_planes(self):
        import torch

        return [torch.empty(s, dtype=self.dtype, device="cuda") for s in self.shapes]

    def reconstruct(self, residue, motion, taps=None):
        """ccd_inter_reconstruct of two device float outputs against the case's references."""
        import torch

        from cool_chic_amd._lib import check, lib

        out = self.new_planes()

        def ptrs(planes):
            return (C.c_void_p * 3)(*[p.data_ptr() for p in planes])

        st = torch.cuda.current_stream().cuda_stream
        check(lib().ccd_inter_reconstruct(0, C.c_void_p(st or None), self.frame_type, self.H, self.W, self.bd, self.fdt,
                                          C.c_void_p(residue.data_ptr()), C.c_void_p(motion.data_ptr()), ptrs(self.refs[0]),
                                          ptrs(self.refs[1]) if self.frame_type == 2 else None, (C.c_int32 * 4)(*self.gflow),
                                          self.taps if taps is None else taps, ptrs(out)), "ccd_inter_reconstruct")
        return out

    def sse(self, role, lats, partner=None):
        """Exact SSE against the source of the frame reconstructed from each latent set of `role` and the partner's output."""
        from cool_chic_amd.quality import QualityMeter

        other = ROLES[1 - ROLES.index(role)]
        partner = self.out[other] if partner is None else partner
        cc, out = self.cc[role], []
        with QualityMeter(0) as meter:
            for i in range(0, len(lats), cc.N):
                outs = cc.outputs(lats[i:i + cc.N])
                planes = [self.reconstruct(o, partner) if role == "residue" else self.reconstruct(partner, o) for o in outs]
                q = meter.score_planes(planes, [self.src] * len(planes), [self.bd] * len(planes), [FDT_NAMES[self.fdt]] * len(planes),
                                       ms_ssim=False)
                out += [sum(int(v) for v in r.sse) for r in q]
        return out

    def brute(self, role, moves, lat=None, partner=None):
        """[(g, y, x, s)] -> SSE(moved) - SSE(base), or SENTINEL where the move leaves the alphabet."""
        lat = self.cc[role].lat if lat is None else lat
        cands, legal = [lat], []
        for g, y, x, s in moves:
            ok = -64 <= int(lat[g][y, x]) + s <= 63
            legal.append(ok)
            if ok:
                l2 = list(lat)
                l2[g] = lat[g].copy()
                l2[g][y, x] += s
                cands.append(l2)
        sse = self.sse(role, cands, partner)
        it = iter(sse[1:])
        return [next(it) - sse[0] if ok else SENTINEL for ok in legal]

    def add_to(self, handle, role, lat_dev=None, partner=None):
        """The role's candidate as a slot of a DistortionDeltas handle."""
        other = ROLES[1 - ROLES.index(role)]
        cc = self.cc[role]
        lat_dev = cc.lat_dev if lat_dev is None else lat_dev
        partner = self.out[other] if partner is None else partner
        return handle.add_inter(cc.arch, cc.nn, cc.ptrs(lat_dev), [t.data_ptr() for t in self.src], self.bd, self.fdt, self.frame_type,
                                ROLES.index(role), partner.data_ptr(), [t.data_ptr() for t in self.refs[0]],
                                [t.data_ptr() for t in self.refs[1]] if self.frame_type == 2 else None, self.gflow, self.taps,
                                owner=(lat_dev, partner, self.src, self.refs))

    def read_maps(self, handle, slot, role):
        import torch

        return [torch.as_tensor(handle.delta_map(slot, g), device="cuda").cpu().numpy() for g in range(self.cc[role].n)]

    def maps(self, role, n_probe_slots=16):
        """The maps of a handle that holds the role's candidate alone."""
        from cool_chic_amd import DistortionDeltas

        if role not in self._maps:
            d = DistortionDeltas(0, n_probe_slots)
            self.add_to(d, role)
            d.run(); d.wait()
            m = self.read_maps(d, 0, role)
            d.close()
            cc = self.cc[role]
            for g, a in enumerate(m):
                assert a.shape == (2,) + cc.hw[g] and a.dtype == np.int64
            self._maps[role] = m
        return self._maps[role]


_CASES = {}


def case(name, coding_index, **kw):
    key = (name, coding_index, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = InterCase(name, coding_index, **kw)
    return _CASES[key]
