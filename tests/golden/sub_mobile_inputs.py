"""Inputs of the GAN-Compression GauGAN fixture (tests/golden/gaugan_sub_mobile.npz), shared by its generator (which feeds them to
the REFERENCE's SIGEFusedSubMobileSPADEGenerator in the build container) and by the tests (which feed them to sige_amd's
SubMobileSpadeGenerator)."""
import torch

from .model_init import gaugan_labels, init_by_name
from .pd_inputs import tile_counts  # noqa: F401

# group -> (config string, ngf, crop_size, (H, W), num_sparse_layers, pixel step of what is stored; None = model_init.summarize)
GROUPS = {
    "small5": ("8_8_8_12_8_8_8_8", 16, 256, (128, 256), 5, 2),    # tiled and dense layers
    "small7": ("8_8_8_12_8_8_8_8", 16, 256, (128, 256), 7, 2),    # every block tiled, down to 2 x 4
    "readme": ("32_32_32_48_32_24_24_32", 64, 512, (256, 512), 4, None),  # the reference's README configuration
}


def channels(config_str: str):
    return tuple(int(c) for c in config_str.split("_"))


def init_weights(model: torch.nn.Module, seed: int = 0) -> None:
    """init_by_name, then the pointwise convs of the separable gamma / beta branches (`.conv.2.` weights and biases) times 0.1 and
    every conv_0 / conv_1 weight times 0.5.  Plain init_by_name weights saturate this model: the InstanceNorm rescales every label
    branch to unit variance, the pre-tanh output has std 23 and 86 % of the outputs lie beyond +-0.99 -- a fixture of +-1 pins
    nothing.  With the damping the output std is 0.23 (README configuration) / 0.145 (small) and nothing lies beyond 0.99."""
    init_by_name(model, seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if ".conv.2." in name:
                p.mul_(0.1)
            elif name.endswith("conv_0.weight") or name.endswith("conv_1.weight"):
                p.mul_(0.5)


def labels(group: str, variant: int = 0):
    """(original, edited) one-hot label maps of a group; `variant` != 0: another original / edit pair of the same size."""
    H, W = GROUPS[group][3]
    return gaugan_labels(H, W, seed=3 + 7 * variant)
