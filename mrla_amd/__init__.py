"""mrla_amd -- MI355X-native MRLA (multi-head recurrent layer attention) hot path.

The compute path is libmrla_hip.so (hand-written HIP for gfx950, C ABI in include/mrla_hip.h); this
package is the host-side mirror of the reference's nn.Module surface on top of it.
"""


def __getattr__(name):
    # (lazy: importing the package must not import torch-heavy modules or load the library)
    if name in ("graphed_step", "GraphedStep", "replay_matches_eager", "capture_step", "GraphReplayMismatch"):
        from . import graphs
        return getattr(graphs, name)
    if name == "fp32_gemms":       # the switch of the fp32 1x1-convolution GEMMs (functional.CONV1X1_F32), as a context manager
        from . import functional
        return functional.fp32_gemms
    if name == "conv3x3_wgrad":    # the switch of the own 3x3 weight gradient (functional.CONV3X3_WGRAD), as a context manager
        from . import functional
        return functional.conv3x3_wgrad
    if name == "conv3x3_wgrad_auto":   # ... and of its route by shape, where the library prefers it (functional.CONV3X3_WGRAD_AUTO)
        from . import functional
        return functional.conv3x3_wgrad_auto
    if name == "conv3x3_wgrad_f32":    # ... and of the fp32 3x3 weight gradient outside autocast (functional.CONV3X3_WGRAD_F32)
        from . import functional
        return functional.conv3x3_wgrad_f32
    if name == "conv3x3_fwd":    # the switch of the own 3x3 forward and stride-1 input gradient (functional.CONV3X3_FWD)
        from . import functional
        return functional.conv3x3_fwd
    if name == "conv3x3_dgrad":    # the switch of the own stride-2 3x3 input gradient (functional.CONV3X3_DGRAD)
        from . import functional
        return functional.conv3x3_dgrad
    if name == "conv3x3_dgrad_flip":   # the switch of the stride-1 3x3 input gradient as a stock forward on banked flipped weights
        from . import functional       # (functional.CONV3X3_DGRAD_FLIP)
        return functional.conv3x3_dgrad_flip
    if name == "stem_wgrad":      # the switch of the own stem (7x7 / stride 2) weight gradient (functional.STEM_WGRAD)
        from . import functional
        return functional.stem_wgrad
    if name == "stem_wgrad_f32":      # ... and of the fp32 stem weight gradient outside autocast (functional.STEM_WGRAD_F32)
        from . import functional
        return functional.stem_wgrad_f32
    if name == "reproducible_gradients":      # all of them (the fp32 3x3 and stem ones included): every parameter gradient a function of the step's inputs alone
        from . import functional
        return functional.reproducible_gradients
    raise AttributeError(f"module 'mrla_amd' has no attribute {name!r}")
