"""Synthetic weights for DySample (module cases of dysample_ops.npz and the yolov13*-DySample.yaml models), shared by
tests/golden/make_golden_dysample.py and the tests.  synthdata.synth_tensor would fill the persistent `init_pos` buffer (a state_dict
key) with N(0, 0.1) noise; every module keeps its own init_pos here, every other key goes through synthdata unchanged."""
import synthdata as synth

GAIN = 0.5  # models: as make_golden_v13.py (the reference's fp32 forward stays within 1.4e-6 of its fp64 forward per layer at this gain)
MODULE_GAIN = 1.9  # module cases: offsets of 1.2-2.1 px with the inputs below, so the samples really leave their cell

NAME = "yolov13{}-DySample.yaml"
DYSAMPLE_LAYERS = (10, 15, 19)


def state_dict(own, gain=GAIN, prefix=""):
    """own: the module's / model's state_dict.  Returns synthetic tensors of the same shapes, `init_pos` buffers kept as built."""
    return {k: (v.detach().clone() if k.rsplit(".", 1)[-1] == "init_pos" else synth.synth_tensor(prefix + k, tuple(v.shape), gain=gain))
            for k, v in own.items()}


# (tag, (in_channels, scale, style, groups, dyscope), input shape (B, C, H, W))
CASES = [
    ("lp_c16_g4_5x7", (16, 2, "lp", 4, False), (2, 16, 5, 7)),  # C / groups = 4: below the kernel's 8 channels per group (refused there)
    ("lp_scope_c32_1x1", (32, 2, "lp", 4, True), (1, 32, 1, 1)),
    ("pl_c32_3x9", (32, 2, "pl", 4, False), (1, 32, 3, 9)),
    ("pl_scope_c64_6x4", (64, 2, "pl", 4, True), (2, 64, 6, 4)),
    ("lp_c16_g2_4x6", (16, 2, "lp", 2, False), (1, 16, 4, 6)),
    ("lp_c128_g8_4x6", (128, 2, "lp", 8, False), (1, 128, 4, 6)),
    ("lp_c96_g4_9x16", (96, 2, "lp", 4, False), (1, 96, 9, 16)),
]


def kernel_supports(args):
    c, _, _, groups, _ = args
    return (c // groups) % 8 == 0


def fill(mod, tag):
    """Load the synthetic weights of a module-level case."""
    mod.eval()
    mod.load_state_dict(state_dict(mod.state_dict(), MODULE_GAIN, tag + "."))
    return mod


def case_input(shape):
    """About +-2: with MODULE_GAIN weights the offset conv then moves samples by more than a pixel."""
    b, c, h, w = shape
    return (synth.synth_images(b, h, w, c=c) * 2 - 1) * 2
