#!/usr/bin/env python3
"""Drop-in for the reference's cc_decode.py (cc_decode.py:12-20): same flags, MI355X decode."""
import argparse

from cool_chic_amd.bitstream.decode import decode_video

if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--input", "-i", type=str, help="Bitstream path.")
    parser.add_argument("--output", "-o", type=str, help="Decoded file path.")
    parser.add_argument("--verbosity", type=int, help="Verbosity level.", default=0)
    parser.add_argument("--device", type=int, help="GPU index.", default=0)
    parser.add_argument("--png-level", type=int, choices=(0, 1), default=0,
                        help="PNG output: 0 = literal-only deflate (default), 1 = with LZ77 matches (smaller files).")
    parser.add_argument("--source", type=str, default=None,
                        help="Source of the stream (.png, .ppm or planar .yuv): every decoded frame is scored against it on the GPU.")
    parser.add_argument("--results", type=str, default=None,
                        help="With --source: tab-separated file with the rate, PSNR and MS-SSIM of every frame and of the sequence.")
    parser.add_argument("--rate-breakdown", type=str, default=None, metavar="FILE",
                        help="Tab-separated file with the model bits of every latent grid of every cool-chic (measured on the GPU).")
    parser.add_argument("--no-ms-ssim", action="store_true", help="With --source: PSNR only.")
    args = parser.parse_args()
    if args.results is not None and args.source is None:
        parser.error("--results needs --source")
    decode_video(args.input, decoded_path=args.output, verbosity=args.verbosity, device=args.device,
                 png_level=args.png_level, source_path=args.source, ms_ssim=not args.no_ms_ssim, results_path=args.results,
                 rate_breakdown_path=args.rate_breakdown)
