"""Case builders of tests/test_dependent_deltas.py: a frame R whose planes are a reference (an intra frame of a video fixture, or
one cool-chic of a P / B frame through tests/inter_cases.py), the P / B frames that predict from it, and the brute force the
dependent maps (ccd_dsens_add_dependent) are compared with.

The brute force uses public calls only and never the new kernel: a latent of R is moved on the host, R is decoded
(DecodeBatch.add_latents* for an intra R, InterCase.reconstruct for an inter R), every dependent goes through ccd_inter_reconstruct
against the moved planes, QualityMeter gives the exact integer SSE against the dependent's source, and the base is subtracted.
A dependent's source is InterCase.src, its reconstruction from a second latent set, so that the differences have both signs."""
import ctypes as C

import numpy as np

import inter_cases as ic

SENTINEL = ic.SENTINEL
N_SLOTS = 64


def margin(fdt, taps_list):
    """The margin of a slot with these dependents, as DESIGN.md 4.16 states it (not through the library): W - 1, or W + 2 for
    yuv420, W the widest window per axis - 2 bilinear, 4 bicubic, the filter size for sinc."""
    w = max(int(t) for t in taps_list)
    return w + 2 if fdt == 1 else w - 1


class IntraRef:
    """The intra frame `coding_index` of a fixture as a candidate: the fixture's latents with the alphabet's ends forced at the
    corners and a few positions, 64 given-latent slots that decode to planes.  `formats` = (frame_data_type index, bitdepth)
    replaces the frame's."""

    def __init__(self, name, coding_index=0, seed=0, formats=None):
        import torch

        from cool_chic_amd import DecodeBatch

        fh, ccs, _, _ = ic.parse_video(name)[coding_index]
        assert fh.frame_type == 0 and len(ccs) == 1
        self.name = f"{name}[{coding_index}]"
        self.fdt, self.bd = (int(fh.frame_data_type), int(fh.bitdepth)) if formats is None else formats
        arch, hdr, nn, payload = ccs[0]
        dec = DecodeBatch(0)
        dec.add(hdr, nn, payload, 0, 0)
        dec.run(); dec.wait()
        base = [dec.latent(0, g) for g in range(int(arch.n_grids))]
        dec.close()
        self.cc = ic._CoolChic.__new__(ic._CoolChic)  # the latent sets and their layout, with slots that write planes
        cc = self.cc
        cc.arch, cc.nn, cc.n = arch, nn, int(arch.n_grids)
        cc.hw = [(int(arch.grid_h[g]), int(arch.grid_w[g])) for g in range(cc.n)]
        cc.sizes = [h * w for h, w in cc.hw]
        cc.off = np.concatenate([[0], np.cumsum([(s + 255) // 256 * 256 for s in cc.sizes])]).astype(np.int64)
        rng = np.random.default_rng([seed, 5, len(name)])
        cc.lat = [a.copy() for a in base]
        for a in cc.lat:
            a.flat[0], a.flat[-1] = -64, 63
            where = rng.choice(a.size, size=min(a.size, 4), replace=False)
            a.flat[where] = rng.choice([-64, 63], size=len(where))
        cc.lat2 = [np.clip(a.astype(np.int16) + rng.integers(-2, 3, size=a.shape), -64, 63).astype(np.int8) for a in cc.lat]
        cc.buf = torch.zeros((N_SLOTS, int(cc.off[-1])), dtype=torch.int8, device="cuda")
        cc.batch = DecodeBatch(0)
        for k in range(N_SLOTS):
            cc.batch.add_latents_device(arch, nn, [cc.buf[k].data_ptr() + int(cc.off[g]) for g in range(cc.n)], self.bd, self.fdt, owner=cc.buf)
        cc.lat_dev = torch.from_numpy(cc.flat(cc.lat)).cuda()
        self.arch, self.nn, self.n, self.hw, self.lat = arch, nn, cc.n, cc.hw, cc.lat
        self.H, self.W = int(arch.img_size[0]), int(arch.img_size[1])
        self.src = [p.clone() for p in self.planes([cc.lat2])[0]]
        self.base_planes = [p.clone() for p in self.planes([cc.lat])[0]]

    def planes(self, lats):
        """The device planes (valid until the next call) of up to 64 latent sets."""
        import torch

        cc = self.cc
        assert len(lats) <= N_SLOTS
        host = np.stack([cc.flat(l) for l in lats] + [cc.flat(lats[0])] * (N_SLOTS - len(lats)))
        cc.buf.copy_(torch.from_numpy(host))
        torch.cuda.synchronize()
        cc.batch.run(); cc.batch.wait()
        return [[torch.as_tensor(cc.batch.plane_device(k, p), device="cuda") for p in range(3)] for k in range(len(lats))]

    def add_to(self, handle, lat_dev=None):
        lat_dev = self.cc.lat_dev if lat_dev is None else lat_dev
        return handle.add(self.arch, self.nn, self.cc.ptrs(lat_dev), [t.data_ptr() for t in self.src], self.bd, self.fdt,
                          owner=(lat_dev, self.src))


class InterRef:
    """One cool-chic (`role`) of a P / B frame as a candidate whose frame is a reference of later frames."""

    def __init__(self, case, role):
        self.case, self.role = case, role
        self.cc = case.cc[role]
        self.name = f"{case.name} {role}"
        self.fdt, self.bd, self.H, self.W = case.fdt, case.bd, case.H, case.W
        self.arch, self.nn, self.n, self.hw, self.lat = self.cc.arch, self.cc.nn, self.cc.n, self.cc.hw, self.cc.lat
        self.base_planes = case.base_planes

    def planes(self, lats):
        other = self.case.out[ic.ROLES[1 - ic.ROLES.index(self.role)]]
        outs = self.cc.outputs(lats)
        return [self.case.reconstruct(o, other) if self.role == "residue" else self.case.reconstruct(other, o) for o in outs]

    def add_to(self, handle, lat_dev=None):
        return self.case.add_to(handle, self.role, lat_dev=lat_dev)


class Dependent:
    """A P / B frame (an InterCase: its two float outputs, its references, its source) that predicts from R as its reference
    `which`.  `motion` / `gflow` replace the frame's flows and global flow."""

    def __init__(self, case, which, motion=None, gflow=None):
        self.case, self.which = case, int(which)
        self.residue = case.out["residue"]
        self.motion = case.out["motion"] if motion is None else motion
        self.gflow = list(case.gflow) if gflow is None else [int(v) for v in gflow]
        self.src = case.src
        assert self.which == 0 or case.frame_type == 2

    def reconstruct(self, ref_planes, motion=None):
        """ccd_inter_reconstruct of the dependent with `ref_planes` in place of its reference `which`."""
        import torch

        from cool_chic_amd._lib import check, lib

        c = self.case
        refs = [c.refs[0], c.refs[1] if c.frame_type == 2 else None]
        refs[self.which] = ref_planes
        out = c.new_planes()

        def ptrs(planes):
            return (C.c_void_p * 3)(*[p.data_ptr() for p in planes])

        st = torch.cuda.current_stream().cuda_stream
        motion = self.motion if motion is None else motion
        check(lib().ccd_inter_reconstruct(0, C.c_void_p(st or None), c.frame_type, c.H, c.W, c.bd, c.fdt, C.c_void_p(self.residue.data_ptr()),
                                          C.c_void_p(motion.data_ptr()), ptrs(refs[0]), ptrs(refs[1]) if c.frame_type == 2 else None,
                                          (C.c_int32 * 4)(*self.gflow), c.taps, ptrs(out)), "ccd_inter_reconstruct")
        return out

    def add_to(self, handle, slot, motion=None):
        c = self.case
        motion = self.motion if motion is None else motion
        other = c.refs[1 - self.which] if c.frame_type == 2 else None
        handle.add_dependent(slot, c.frame_type, self.which, self.residue.data_ptr(), motion.data_ptr(), [t.data_ptr() for t in self.src],
                             None if other is None else [t.data_ptr() for t in other], self.gflow, c.taps,
                             owner=(self.residue, motion, self.src, other))


def brute(ref, deps, moves, lat=None, motions=None):
    """[(g, y, x, s)] -> sum over the dependents of SSE_F(R moved) - SSE_F(R as decoded); SENTINEL where the move leaves the
    alphabet."""
    from cool_chic_amd.quality import QualityMeter

    lat = ref.lat if lat is None else lat
    cands, legal = [lat], []
    for g, y, x, s in moves:
        ok = -64 <= int(lat[g][y, x]) + s <= 63
        legal.append(ok)
        if ok:
            l2 = list(lat)
            l2[g] = lat[g].copy()
            l2[g][y, x] += s
            cands.append(l2)
    names = [ic.FDT_NAMES[ref.fdt]]
    total = []
    with QualityMeter(0) as meter:
        for i in range(0, len(cands), N_SLOTS):
            planes = ref.planes(cands[i:i + N_SLOTS])
            part = [0] * len(planes)
            for q, dep in enumerate(deps):
                rec = [dep.reconstruct(p, None if motions is None else motions[q]) for p in planes]
                res = meter.score_planes(rec, [dep.src] * len(rec), [ref.bd] * len(rec), names * len(rec), ms_ssim=False)
                for k, r in enumerate(res):
                    part[k] += sum(int(v) for v in r.sse)
            total += part
    it = iter(total[1:])
    return [next(it) - total[0] if ok else SENTINEL for ok in legal]


def run_maps(handle_cls, ref, deps, n_probe_slots=16, extra=None):
    """(own maps, dependent maps, conflicts per grid, passes) of a handle that holds R with `deps`."""
    import torch

    d = handle_cls(0, n_probe_slots)
    if extra is not None:
        extra(d)
    slot = ref.add_to(d)
    for dep in deps:
        dep.add_to(d, slot)
    d.run(); d.wait()
    own = [torch.as_tensor(d.delta_map(slot, g), device="cuda").cpu().numpy() for g in range(ref.n)]
    dep_maps = [torch.as_tensor(d.dep_delta_map(slot, g), device="cuda").cpu().numpy() for g in range(ref.n)] if deps else None
    conflicts = [d.dep_conflicts(slot, g) for g in range(ref.n)] if deps else None
    passes = d.passes(slot)
    d.close()
    return own, dep_maps, conflicts, passes


def expected_passes(ref, m):
    from cool_chic_amd.dsens import probe_stride

    n = 0
    for g in range(ref.n):
        s = probe_stride(ref.arch, g, ref.fdt, margin=m)
        n += 2 * min(s, ref.hw[g][0]) * min(s, ref.hw[g][1]) if s else 0
    return n


def tap_offsets(motion, which, H, W, taps):
    """The integer tap offsets of a sinc warp's flows for reference `which` (floor of the flow after the saturation of
    ic_tap_offset): [2][H][W] int64 (rows, columns), from a downloaded motion output."""
    fx, fy = motion[2 * which], motion[2 * which + 1]
    oy = np.clip(np.floor(fy), -(H + 16), H + 16).astype(np.int64)
    ox = np.clip(np.floor(fx), -(W + 16), W + 16).astype(np.int64)
    return np.stack([oy, ox])


def quad_spread(off):
    """Largest difference of the offsets inside any 2 x 2 quad, per axis."""
    a = off.reshape(2, off.shape[1] // 2, 2, off.shape[2] // 2, 2)
    return int((a.max(axis=(2, 4)) - a.min(axis=(2, 4))).max())


_CACHE = {}


def intra(name, coding_index=0, **kw):
    key = (name, coding_index, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = IntraRef(name, coding_index, **kw)
    return _CACHE[key]
