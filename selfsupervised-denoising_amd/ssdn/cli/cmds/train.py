"""`ssdn train start|resume` (same flags as /root/reference/ssdn/ssdn/cli/cmds/train.py:18-188).  Reference defects fixed
(SURVEY.md Appendix A): `--mono` only switches to one channel when given (the reference always did, cmds/train.py:153-154);
`--diagonal` sets DIAGONAL_COVARIANCE (the reference overwrote TRAIN_ITERATIONS with it, :155-156) and trains the SSDN model with a
diagonal posterior covariance (the reference's own diagonal branch raises at `c00.shape()`, denoiser.py:240; this build's head is
DESIGN.md section 3.10; the MSE pipelines ignore the flag, as the reference does); `resume` edits the loaded trainer's cfg (the
reference used an undefined `cfg`, :168-181)."""
from typing import Dict

import ssdn
from ssdn.cfg import DEFAULT_RUN_DIR
from ssdn.cli.cmds.cmd import Command
from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue

_SHARED = (("iterations", ConfigValue.TRAIN_ITERATIONS), ("eval_interval", ConfigValue.EVAL_INTERVAL),
           ("checkpoint_interval", ConfigValue.SNAPSHOT_INTERVAL), ("print_interval", ConfigValue.PRINT_INTERVAL),
           ("train_batch_size", ConfigValue.TRAIN_MINIBATCH_SIZE), ("validation_batch_size", ConfigValue.TEST_MINIBATCH_SIZE),
           ("patch_size", ConfigValue.TRAIN_PATCH_SIZE))


def _positive_int(text: str) -> int:
    import argparse
    try:
        v = int(text)
    except ValueError:
        v = 0
    if v < 1:
        raise argparse.ArgumentTypeError("expected an integer >= 1, got %r" % text)
    return v


class TrainCommand(Command):
    START_CMD, RESUME_CMD = "start", "resume"

    def cmd(self) -> str:
        return "train"

    def configure(self, parser):
        p = parser.add_parser(self.cmd(), help="Train or resume training of a Denoiser model.")
        actions = p.add_subparsers(dest="train_cmd", required=True)
        s = actions.add_parser(self.START_CMD, help="start a new training run")
        self._shared(s, True)
        s.add_argument("--algorithm", "-a", required=True, choices=[c.value for c in NoiseAlgorithm], help="The algorithm to train.")
        s.add_argument("--noise_style", "-n", required=True,
                       help="'gauss{SD}', 'gauss{MIN}_{MAX}', 'poisson{LAMBDA}', 'poisson{MIN}_{MAX}', 'impulse{A}', 'impulse{LO}_{HI}'; "
                            "integer gauss values are /255, integer impulse values are per cent ('impulse50': half of the pixels replaced; "
                            "with a decimal point: fractions); append '_nc' to disable clipping (no effect on impulse).")
        s.add_argument("--noise_value", choices=[c.value for c in NoiseValue], help="[SSDN] Whether the noise value should be estimated.")
        s.add_argument("--mono", action="store_true", help="Convert input data to greyscale (single channel).")
        s.add_argument("--diagonal", action="store_true", help="[SSDN] Enforce a diagonal covariance matrix.")
        s.add_argument("--runs_dir", default=DEFAULT_RUN_DIR, help="Directory in which the output directory is generated.")
        s.add_argument("--noisy", nargs="?", const="style", choices=["style", "auto"], metavar="style|auto",
                       help="[ssdn, ssdn_u_only, n2v] The training images are ALREADY noisy: no noise is added, they are decoded once into a "
                            "device-resident pool and every minibatch is cut out of it on the device. 'style' (the default): they carry the "
                            "corruption --noise_style describes, its number is the known parameter. 'auto' (ssdn, --noise_value known, gauss "
                            "or poisson): the parameter of every image is estimated when the pool is built. The validation set, if any, "
                            "still holds clean images. A resumed run continues in the mode it was started with.")
        s.add_argument("--augment", action="store_true",
                       help="[--noisy] Apply one of the eight flips / transpositions of the square, drawn per sample, to every patch.")
        s.add_argument("--pool_gb", type=float, metavar="G", help="[--noisy] Cap of the device-resident image pool in GiB (default 8).")
        s.add_argument("--white", type=int, metavar="W",
                       help="[--noisy, 16-bit training images] The sample value that means 1.0: an integer in [1, 65535], default 65535; 4095 "
                            "for 12-bit camera files. The noise style's number is in units of white / 255.")
        s.add_argument("--noisy_validation", metavar="PATH",
                       help="[--noisy; ssdn with a gauss or poisson style] A folder or file of held-out images that are already noisy, of the "
                            "pool's depth: at every eval_interval they are denoised and scored WITHOUT clean images -- psnr_out_est, "
                            "psnr_mu_est (PSNR estimated from the noisy image alone) and nll_noisy in the VALID line and the valid/ scalars, "
                            "the first output under val_imgs/. Independent of -v. A resumed run continues it.")
        r = actions.add_parser(self.RESUME_CMD, help="Resume the training of a model from the latest *.training file of a run directory.")
        r.add_argument("run_dir", help="Path to run directory to resume.")
        self._shared(r, False)

    @staticmethod
    def _shared(p, start: bool):
        p.add_argument("--train_dataset", "-t", required=start, help="hdf5 file generated by 'dataset_tool_h5.py' or a folder of images.")
        p.add_argument("--validation_dataset", "-v", help="hdf5 file or folder of images.")
        p.add_argument("--iterations", "-i", required=start, type=int, help="Number of iterations (input images) to train for.")
        for name in ("eval_interval", "checkpoint_interval", "print_interval", "train_batch_size", "validation_batch_size", "patch_size"):
            p.add_argument("--" + name, type=int)
        p.add_argument("--accumulate", type=_positive_int, metavar="K",
                       help="Minibatches per optimiser step: the gradients of K minibatches are summed on the device and Adam steps once on "
                            "their mean (effective batch K x train_batch_size; one gradient exchange per step in multi-GPU runs). "
                            "Default 1; a resumed run keeps the value it was started with.")

    def execute(self, args: Dict):
        from ssdn.train import DenoiserTrainer, resume_run
        if args["train_cmd"] == self.START_CMD:
            if args["algorithm"] == "ssdn" and args.get("noise_value") is None:
                args["PARSER"].error("SSDN requires --noise_value")
            cfg = ssdn.cfg.base()
            cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm(args["algorithm"])
            cfg[ConfigValue.NOISE_STYLE] = args["noise_style"]
            if args.get("noise_value") is not None:
                cfg[ConfigValue.NOISE_VALUE] = NoiseValue(args["noise_value"])
            if args.get("mono"):
                cfg[ConfigValue.IMAGE_CHANNELS] = 1
            if args.get("diagonal"):
                cfg[ConfigValue.DIAGONAL_COVARIANCE] = True
            trainer = DenoiserTrainer(cfg, runs_dir=args["runs_dir"])
        elif args["train_cmd"] == self.RESUME_CMD:
            trainer = resume_run(args["run_dir"])
            cfg = trainer.cfg
        else:
            raise NotImplementedError("Invalid train command")
        if args.get("train_dataset") is not None:
            trainer.set_train_data(args["train_dataset"])
        if args.get("validation_dataset") is not None:
            trainer.set_test_data(args["validation_dataset"])
        for name, key in _SHARED:
            if args.get(name) is not None:
                cfg[key] = args[name]
        if args.get("accumulate") is not None:
            trainer.accumulate = args["accumulate"]
        if args["train_cmd"] == self.START_CMD:
            from ssdn.train import check_noisy
            trainer.noisy, trainer.augment = args.get("noisy"), bool(args.get("augment"))
            trainer.pool_bytes = int(args["pool_gb"] * 2 ** 30) if args.get("pool_gb") is not None else None
            trainer.white = args.get("white")
            trainer.noisy_validation = args.get("noisy_validation")
            try:
                check_noisy(cfg, trainer.noisy, trainer.augment, trainer.pool_bytes, trainer.white, trainer.noisy_validation)
            except ValueError as e:
                args["PARSER"].error(str(e))
        trainer.train()
        return trainer
