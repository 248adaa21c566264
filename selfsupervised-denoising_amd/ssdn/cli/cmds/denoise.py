"""`ssdn denoise --model M --input I --output O [--noise_param P|auto] [--batch_size B] [--bucket N] [--uniform] [--std] [--recursive]
[--tile T] [--overlap O] [--white W] [--risk [--risk_margin M]]`:
denoise already noisy images with a trained model (the reference has no such command: its evaluator takes clean datasets and adds
the noise itself).  I: an image file or a folder of images (file discovery and channel conversion of datasets/folder.py); writes
O/<relative stem>.png, with --std O/<relative stem>_std.npy (float32 [C,h,w] posterior std dev, ssdn models only), and O/denoise.csv
with one row per image (with --noise_param auto also the noise parameter estimated for it, with --tile also the number of tiles it was
cut into).  A 16-bit grey file (ssdn.utils.load_image) comes back as a 16-bit grey PNG; --white W is the sample value that means 1.0 in such
files (default 65535; 4095 for a 12-bit camera file).  --risk (ssdn models with a gauss or poisson style) adds the columns psnr_out_est,
psnr_mu_est, nll and clipped to denoise.csv -- a PSNR estimated from the noisy image alone (`Denoiser.risk`) -- and a last log line with
their mean.  PNG decode and encode stay on the host
with PIL; everything between is `Denoiser.denoise`."""
import os
from typing import Dict, List, Tuple

from ssdn.cli.cmds.cmd import Command


def find_images(path: str, recursive: bool = False) -> Tuple[str, List[str]]:
    """-> (the directory relative stems are taken from, the image files under `path` in the order of UnlabelledImageFolderDataset)"""
    from ssdn.datasets.folder import UnlabelledImageFolderDataset, is_image_file
    path = os.path.expanduser(path)
    if os.path.isfile(path):
        if not is_image_file(path):
            raise ValueError("denoise: %s is not an image file" % path)
        return os.path.dirname(path), [path]
    if not os.path.isdir(path):
        raise FileNotFoundError("denoise: no such file or folder: %s" % path)
    return path, UnlabelledImageFolderDataset(path, recursive=recursive).files


class DenoiseCommand(Command):
    def cmd(self) -> str:
        return "denoise"

    def configure(self, parser):
        p = parser.add_parser(self.cmd(), help="Denoise noisy images with a pre-trained model.")
        p.add_argument("--model", "-m", required=True, help="Path to model weights (.wt) or training file (.training).")
        p.add_argument("--input", "-i", required=True, help="A noisy image file or a folder of noisy images.")
        p.add_argument("--output", "-o", required=True, help="Directory the denoised PNGs and denoise.csv are written to.")
        p.add_argument("--noise_param", default=None,
                       help="The noise parameter of the images, for ssdn models trained with a known one: the numeric part of the "
                            "noise style (gauss: an integer is /255; poisson: lambda; impulse: an integer is per cent), or "
                            "'auto' (gauss and poisson models): estimate it per image on the device; denoise.csv then gains a "
                            "noise_param column with the value used.")
        p.add_argument("--batch_size", type=int, default=1, help="Images of one padded shape per batch.")
        p.add_argument("--bucket", type=int, default=None,
                       help="Pad every image to a multiple of this (a multiple of 32; default 32): fewer distinct plans for more padding.")
        p.add_argument("--uniform", action="store_true", help="Pad every image to the largest one (one plan for the whole folder).")
        p.add_argument("--std", action="store_true",
                       help="Also write <stem>_std.npy: the per-pixel posterior std dev, float32 [C,h,w] (ssdn models only).")
        p.add_argument("--recursive", action="store_true", help="Also take the images of the folder's sub-folders.")
        p.add_argument("--tile", type=int, default=None,
                       help="Denoise every image wider or taller than this (a multiple of 32) in overlapping tiles of this edge through one "
                            "plan: images of any size in bounded memory; denoise.csv then gains a tiles column.")
        p.add_argument("--overlap", type=int, default=None,
                       help="The overlap of neighbouring tiles (a multiple of 32, at most half of --tile; default a quarter of it).")

        p.add_argument("--white", type=int, default=None,
                       help="The sample value that means 1.0 in 16-bit input files (an integer in [1, 65535], default 65535; 4095 for a "
                            "12-bit camera file).  Only with 16-bit inputs, which are written back as 16-bit grey PNGs.")

        p.add_argument("--risk", action="store_true",
                       help="Also estimate, from each noisy image alone, the PSNR of the output (psnr_out_est) and of the prior mean "
                            "(psnr_mu_est) against the clean image nobody has, and the negative log-likelihood of the noisy pixels under the "
                            "model (nll): four more columns of denoise.csv (with clipped, the share of samples at 0 or 1, where the noise "
                            "is not zero-mean).  ssdn models with a gauss or poisson style; not with --tile.  The estimate inherits an error "
                            "of --noise_param: a sigma that is too large reads as a better PSNR.  A small image gives a noisy estimate, "
                            "possibly NaN.")
        p.add_argument("--risk_margin", type=int, default=16,
                       help="Leave this many pixels on every side of an image out of --risk (default 16): next to a reflection-padded edge "
                            "a pixel has a copy of itself inside the network's field of view and the estimate is optimistic.")

    RISK_COLUMNS = ("psnr_out_est", "psnr_mu_est", "nll", "clipped")

    def execute(self, args: Dict):
        import logging
        import math
        import numpy as np
        import torch
        from PIL import Image
        from ssdn.denoiser import Denoiser
        from ssdn.params import ConfigValue
        from ssdn.utils.data import load_image, save_image16
        sd = torch.load(args["model"], map_location="cpu", weights_only=False)
        denoiser = Denoiser.from_state_dict(sd["denoiser"] if "denoiser" in sd else sd)
        channels = denoiser.cfg[ConfigValue.IMAGE_CHANNELS]
        opts = dict(noise_param=args.get("noise_param"), batch_size=args.get("batch_size") or 1, bucket=args.get("bucket"),
                    uniform=bool(args.get("uniform")), std=bool(args.get("std")), tile=args.get("tile"), overlap=args.get("overlap"))
        if args.get("risk"):                            # (off: the call, the result and the files are what they are without the flags)
            opts.update(risk=True, risk_margin=args.get("risk_margin") if args.get("risk_margin") is not None else 16)
        denoiser.denoise([], **opts)                    # (the model's refusals, before a file is opened or a directory made)
        base, files = find_images(args["input"], bool(args.get("recursive")))
        images = []
        for path in files:
            a = load_image(path, channels)
            images.append(a[:, :, 0] if a.shape[2] == 1 else a)
        res = denoiser.denoise(images, white=args.get("white"), **opts)
        out_dir = args["output"]
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "denoise.csv"), "w") as csv:
            csv.write(",".join(["file", "width", "height"] + (["noise_std"] if "noise_std" in res else [])
                               + (["noise_param"] if "noise_param" in res else []) + (["tiles"] if "tiles" in res else [])
                               + (list(self.RISK_COLUMNS) if "risk" in res else [])) + "\n")
            for k, path in enumerate(files):
                stem = os.path.splitext(os.path.relpath(path, base))[0]
                os.makedirs(os.path.dirname(os.path.join(out_dir, stem)) or out_dir, exist_ok=True)
                if res["out"][k].dtype == torch.uint16:
                    save_image16(res["out"][k], os.path.join(out_dir, stem + ".png"))
                else:
                    Image.fromarray(res["out"][k].numpy()).save(os.path.join(out_dir, stem + ".png"))
                if "std" in res:
                    np.save(os.path.join(out_dir, stem + "_std.npy"), res["std"][k].numpy().astype(np.float32))
                h, w = images[k].shape[:2]
                csv.write(",".join([os.path.relpath(path, base), str(w), str(h)]
                                   + (["{:.6f}".format(res["noise_std"][k])] if "noise_std" in res else [])
                                   + (["{:.9g}".format(res["noise_param"][k])] if "noise_param" in res else [])
                                   + ([str(res["tiles"][k])] if "tiles" in res else [])
                                   + (["{:.6f}".format(res["risk"][k][c]) for c in self.RISK_COLUMNS] if "risk" in res else [])) + "\n")
        if "risk" in res:
            est = [r["psnr_out_est"] for r in res["risk"]]
            good = [v for v in est if not math.isnan(v)]
            logging.getLogger("ssdn.denoise").info(
                "RISK psnr_out_est=%s dB (mean over %d of %d images; %d without an estimate: NaN)"
                % ("%.4f" % (sum(good) / len(good)) if good else "nan", len(good), len(est), len(est) - len(good)))
        return res
