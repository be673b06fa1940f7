"""Small host-side helpers."""
from __future__ import annotations

import contextlib

import torch


@contextlib.contextmanager
def no_init():
    """Skip torch's default parameter initialisation while constructing modules whose weights are about to be
    overwritten (checkpoint load / synthetic fill): the 194 M-parameter UNet otherwise spends ~10 s in kaiming_uniform_."""
    names = ("kaiming_uniform_", "uniform_", "normal_", "trunc_normal_", "xavier_uniform_", "zeros_", "ones_")
    saved = {n: getattr(torch.nn.init, n) for n in names}
    try:
        for n in names:
            setattr(torch.nn.init, n, lambda t, *a, **k: t)
        yield
    finally:
        for n, f in saved.items():
            setattr(torch.nn.init, n, f)


def add_guidance_arguments(ap) -> None:
    """the command-line form of DiffusionPipeline's guidance stage (scripts/sample.py, sample_dataset.py, img2img.py, edit.py)"""
    ap.add_argument("--guidance-rescale", type=float, default=0.0, metavar="PHI",
                    help="guidance rescale: bring the guided prediction's per-sample spread back towards the conditional one's, weight in [0, 1]")
    ap.add_argument("--dynamic-threshold", type=float, default=None, metavar="Q",
                    help="dynamic thresholding: clamp the x_0 estimate to its per-sample Q-quantile of |x_0| (at least 1) and divide by it, Q in (0, 1]")
    ap.add_argument("--threshold-max", type=float, default=None, metavar="S", help="cap of the dynamic threshold, > 1")
    ap.add_argument("--guidance-interval", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="guide only at timesteps LO <= t <= HI (scale 1 elsewhere; both passes still run)")


def guidance_kwargs(args) -> dict:
    """the keywords of sample() / sample_from() / edit() for the arguments above; empty when none was given (the call is the plain call)"""
    kw = {}
    if args.guidance_rescale:
        kw["guidance_rescale"] = args.guidance_rescale
    if args.dynamic_threshold is not None:
        kw["dynamic_threshold"] = args.dynamic_threshold
    if args.threshold_max is not None:
        kw["threshold_max"] = args.threshold_max
    if args.guidance_interval is not None:
        kw["guidance_schedule"] = ("interval", args.guidance_interval[0], args.guidance_interval[1])
    return kw
