"""`DenoiserEvaluator` -- evaluation driver (drop-in for /root/reference/ssdn/ssdn/eval.py:18-125): load a `.wt` or `.training`
file, pad every test image by reflection to a x32 multiple / square / uniform size (Kodak 768x768, BSD300 512x512), run the
forward kernels, un-pad, per-image PSNR -> `psnrs.csv` (with `ssim` set: per-image SSIM -> `ssims.csv`; with `calibration` set:
per-image reference-free risk estimate with `risk` set -> `risk.csv`; per-image posterior calibration -> `calibration.csv`, the z-score histogram of the whole evaluation -> `calibration_hist.csv`), images -> `eval_imgs/`.  Reference defect fixed: `runs_dir` is honoured
(eval.py:32-35 drops it)."""
import logging
import os
from typing import Callable, Dict

import torch

import ssdn
from ssdn.cfg import DEFAULT_RUN_DIR
from ssdn.datasets import NoisyDataset
from ssdn.denoiser import Denoiser
from ssdn.params import PipelineOutput
from ssdn.train import _CALIB_CACHE, _RISK_CACHE, _SSIM_CACHE, DenoiserTrainer

logger = logging.getLogger("ssdn.eval")


class DenoiserEvaluator(DenoiserTrainer):
    RUN_KIND = "eval"

    def __init__(self, target_path: str, runs_dir: str = DEFAULT_RUN_DIR, run_dir: str = None):
        super().__init__({}, runs_dir=runs_dir)
        sd = torch.load(target_path, map_location="cpu", weights_only=False)
        if "denoiser" in sd:
            self.load_state_dict(sd)
        else:
            self.denoiser = Denoiser.from_state_dict(sd)
        self.cfg = self.denoiser.cfg
        self._run_dir = run_dir
        # `ssdn eval --posterior N`: None = off; N >= 0: per image of the first pass, the posterior std map and N posterior samples
        self.posterior_samples = None
        self.init_state()

    def evaluate(self):
        self.reset_metrics(train=False)
        if self.denoiser is None:
            raise RuntimeError("Denoiser not initialised for evaluation")
        _ = self.writer
        ssdn.logging_helper.setup(self.run_dir_path, "log.txt")
        logger.info("Loading Test Dataset...")
        self.testloader, self.testset, self.test_sampler = self.test_data()
        logger.info(ssdn.utils.separator())
        logger.info("EVALUATION STARTED")
        self._evaluate(self.testloader, self.evaluation_output_callback(self.testset))
        if self.calibration and self.calibration_hist is not None:
            self.save_calibration_hist()
        logger.info(self.eval_state_str("EVALUATION RESULT"))
        logger.info("EVALUATION FINISHED")
        logger.info(ssdn.utils.separator())
        return {k: float(torch.as_tensor(m.accumulated()).float().mean())
                for k, m in self.state[ssdn.params.StateValue.HISTORY][ssdn.params.HistoryValue.EVAL].items()
                if isinstance(m, ssdn.utils.Metric) and not m.empty()}

    def evaluation_output_callback(self, dataset) -> Callable[[int, Dict], None]:
        """psnrs.csv gets a row for EVERY evaluated instance; images are saved for the first pass over the dataset only
        (the test sets are evaluated several times with fresh noise, cfg.test_length)."""
        def callback(output_0_index: int, outputs: Dict):
            inp = outputs[PipelineOutput.INPUTS][NoisyDataset.INPUT]
            metadata = outputs[PipelineOutput.INPUTS][NoisyDataset.METADATA]
            n = inp.shape[0]
            remaining = len(dataset) - output_0_index
            if remaining > 0:
                self.save_image_outputs(outputs, os.path.join(self.run_dir_path, "eval_imgs"), "img_{index:05}_{desc}.png",
                                        batch_indexes=range(min(remaining, n)))
                if self.posterior_samples is not None:
                    self.save_posterior_outputs(outputs, output_0_index, range(min(remaining, n)))
            with open(os.path.join(self.run_dir_path, "psnrs.csv"), "a") as f:
                if output_0_index == 0:
                    f.write(",".join(["id", "psnr_nsy"] + list(self.img_outputs(prefix="psnr").values())) + "\n")
                clean = metadata[NoisyDataset.Metadata.CLEAN]
                pairs = zip(NoisyDataset.unpad(inp.cpu(), metadata), NoisyDataset.unpad(clean, metadata))
                values = [torch.stack([ssdn.utils.calculate_psnr(a, b) for a, b in pairs])]
                values += [self.calculate_psnr(outputs, key, unpad=True).cpu() for key in self.img_outputs(prefix="psnr")]
                for i in range(n):
                    f.write(",".join(["{:04d}".format(output_0_index + i)] + ["{:.4f}".format(float(v[i])) for v in values]) + "\n")
            per = outputs.get(_SSIM_CACHE)
            if per is not None:                 # `ssdn eval --ssim`: the same rows, SSIM instead of PSNR
                names = ["ssim_nsy"] + list(self.img_outputs(prefix="ssim").values())
                with open(os.path.join(self.run_dir_path, "ssims.csv"), "a") as f:
                    if output_0_index == 0:
                        f.write(",".join(["id"] + names) + "\n")
                    for i in range(n):
                        f.write(",".join(["{:04d}".format(output_0_index + i)] + ["{:.6f}".format(float(per[k][i])) for k in names]) + "\n")
            cal = outputs.get(_CALIB_CACHE)
            if cal is not None:                 # `ssdn eval --calibration`: the same rows, the calibration of the posterior covariance
                names = list(ssdn.utils.data.CALIB_VALUES)
                with open(os.path.join(self.run_dir_path, "calibration.csv"), "a") as f:
                    if output_0_index == 0:
                        f.write(",".join(["id"] + names) + "\n")
                    for i in range(n):
                        f.write(",".join(["{:04d}".format(output_0_index + i)] + ["{:.6f}".format(float(cal[k][i])) for k in names]) + "\n")
            rk = outputs.get(_RISK_CACHE)
            if rk is not None:                  # `ssdn eval --risk`: the same rows, the reference-free risk estimate
                names = list(ssdn.utils.data.RISK_VALUES)
                with open(os.path.join(self.run_dir_path, "risk.csv"), "a") as f:
                    if output_0_index == 0:
                        f.write(",".join(["id"] + names) + "\n")
                    for i in range(n):
                        f.write(",".join(["{:04d}".format(output_0_index + i)] + ["{:.6f}".format(float(rk[k][i])) for k in names]) + "\n")
        return callback

    def save_calibration_hist(self) -> None:
        """`calibration_hist.csv`: the z-score histogram summed over the whole evaluation, one row per bin: bin_lo, bin_hi (the two end
        bins reach to -inf / inf), expected = Phi(hi) - Phi(lo) of a standard normal, and per channel the fraction of its z-scores in
        the bin (a calibrated model follows `expected`)."""
        import math
        hist = self.calibration_hist.to(torch.float64)
        frac = hist / hist.sum(1, keepdim=True)
        edges = [-math.inf] + [-4.0 + 0.25 * k for k in range(33)] + [math.inf]
        phi = lambda x: 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))      # noqa: E731
        with open(os.path.join(self.run_dir_path, "calibration_hist.csv"), "w") as f:
            f.write(",".join(["bin_lo", "bin_hi", "expected"] + ["ch{}".format(c) for c in range(hist.shape[0])]) + "\n")
            for k in range(hist.shape[1]):
                lo, hi = edges[k], edges[k + 1]
                f.write(",".join(["{:g}".format(lo), "{:g}".format(hi), "{:.8f}".format(phi(hi) - phi(lo))]
                                 + ["{:.8f}".format(float(frac[c, k])) for c in range(hist.shape[0])]) + "\n")

    def save_posterior_outputs(self, outputs: Dict, output_0_index: int, batch_indexes) -> None:
        """`posterior/img_{index:05}_std.npy` (float32 [C,h,w], un-padded, upright) and `posterior/img_{index:05}_sample{k}.png` for the
        images `eval_imgs/` gets: Denoiser.posterior of the batch just evaluated (its own inference run; the seed is fixed and the offset
        is the batch's first index, so a repeated evaluation draws the same samples)."""
        import numpy as np
        data = outputs[PipelineOutput.INPUTS]
        metadata = data[NoisyDataset.METADATA]
        post = self.denoiser.posterior(data, samples=self.posterior_samples, seed=0, offset=output_0_index)
        out_dir = os.path.join(self.run_dir_path, "posterior")
        os.makedirs(out_dir, exist_ok=True)
        std = post["std"].cpu()
        smp = post["samples"].cpu() if self.posterior_samples else None
        for bi in batch_indexes:
            stem = os.path.join(out_dir, "img_{index:05}".format(index=int(metadata[NoisyDataset.Metadata.INDEXES][bi])))
            # (the dataset classes hand out tensors with H and W swapped, utils/data.py: swapped back here as tensor2image does)
            np.save(stem + "_std.npy", NoisyDataset.unpad(std, metadata, bi).permute(0, 2, 1).contiguous().numpy().astype(np.float32))
            for k in range(self.posterior_samples):
                ssdn.utils.save_tensor_image(NoisyDataset.unpad(smp[k], metadata, bi), stem + "_sample{}.png".format(k))
