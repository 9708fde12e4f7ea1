"""cool_chic_amd - MI355X-native decoder for Cool-chic 5.0 `.cool` bitstreams.

The hot path (integer ARM/IFCE entropy model + range decoder, latent-pyramid upsampling, synthesis,
integer planes) is hand-written HIP for gfx950 in csrc/, behind the C ABI of include/ccd.h; this
package is the thin host-side mirror of the reference's decode surface:

    reference (coolchic.*)                         here (cool_chic_amd.*)
    bitstream.decode.decode_video / decode_frame   bitstream.decode.decode_video / decode_frame
    bitstream.component.coolchic.encode_decode_coolchic(mode="decode")
                                                   bitstream.component.coolchic.encode_decode_coolchic
    bitstream.header.header.{Video,Frame,CoolChic}Header
                                                   bitstream.header.{Video,Frame,CoolChic}Header
    io.io.save_frame_data_to_file, io.framedata.FrameData
                                                   io.save_frame_data_to_file, io.FrameData
    bitstream.encode.encode_frame (range-coding of the latents, encode.py:83-92)
                                                   encoder.EncodeBatch, writer.encode_coolchic(device=...)
    training.loss.loss_function on a candidate (distortion + lmbda * rate, training/loss.py:158)
                                                   rd.RdEvaluator (exact integer ARM and integer planes)
    (no counterpart: what moving one latent by +-1 does to the squared error of the decoded planes)
                                                   dsens.DistortionDeltas, RdEvaluator.cost_delta_map
    (no counterpart: a requantisation step that moves latents by +-1 where the moves provably add)
                                                   rdoq.RdoqStep, RdEvaluator.descend
    (the same for the two cool-chics of a P / B frame, scored through the reconstruction against its references)
                                                   DistortionDeltas.add_inter, rd_inter.InterRdEvaluator
    (intra frames and the residues of the frames that predict from them in one step, claims following the flows)
                                                   RdoqStep.follow, rd_gop.GopDescent
    nnquant.quantizemodel.quantize_model (the search over the networks' quantisation steps, one test pass per candidate)
                                                   nnquant.NetworkQuantiser (every candidate of a module in one batch)
    (the same search for the two cool-chics of a P / B frame: candidates reconstructed and scored on the device, many per launch)
                                                   iscore.InterScore, nnquant_inter.InterNetworkQuantiser
    (no counterpart: a +-1 descent over the ARM's transmitted integers, every candidate's rate change from one table)
                                                   EncodeBatch.measure_param_deltas, nnrefine.ArmRefiner
    (the same over the IFCE's integers, and over both rate networks in one descent)
                                                   EncodeBatch.measure_ifce_deltas, nnrefine.RateRefiner
"""
from ._lib import CcdError, lib  # noqa: F401
from .batch import DecodeBatch  # noqa: F401
from .encoder import EncodeBatch, ParamDeltas  # noqa: F401


def __getattr__(name):
    if name == "RdEvaluator":  # (rd.py needs torch at import: loaded when first asked for)
        from .rd import RdEvaluator

        return RdEvaluator
    if name == "InterRdEvaluator":
        from .rd_inter import InterRdEvaluator

        return InterRdEvaluator
    if name == "GopDescent":
        from .rd_gop import GopDescent

        return GopDescent
    if name == "DistortionDeltas":
        from .dsens import DistortionDeltas

        return DistortionDeltas
    if name == "RdoqStep":
        from .rdoq import RdoqStep

        return RdoqStep
    if name in ("NetworkQuantiser", "QuantisedNetwork"):
        from . import nnquant

        return getattr(nnquant, name)
    if name == "InterScore":
        from .iscore import InterScore

        return InterScore
    if name in ("InterNetworkQuantiser", "QuantisedInterNetworks"):
        from . import nnquant_inter

        return getattr(nnquant_inter, name)
    if name in ("ArmRefiner", "RateRefiner", "RefinedNetwork", "expgol_bit_deltas", "pick_moves"):
        from . import nnrefine

        return getattr(nnrefine, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def pool_trim(device: int = 0) -> None:
    """Returns the device / pinned blocks that destroyed batches left in the library's per-device cache to the HIP runtime
    (include/ccd.h: ccd_pool_trim; caps: CCD_POOL_MAX_MB, CCD_PINNED_POOL_MAX_MB).  The cache is invisible to PyTorch's
    allocator: call this before a memory-hungry torch workload shares the GPU."""
    lib().ccd_pool_trim(int(device))


__version__ = "0.1.0"
