"""CPU: the modules that normalise their rows refuse, where they are constructed, a width the LayerNorm kernels do not take (more
than 4096 columns, or no multiple of 4) -- and construct at every width the kernels do take."""
import pytest
import torch


def _block(dim):
    from afft_amd.models.transformerblock import Block
    return Block(dim, num_heads=4, mlp_ratio=0.25)


def _decoder_block(dim):
    from afft_amd.models.transformerblock import DecoderBlock
    return DecoderBlock(dim, num_heads=4, mlp_ratio=0.25)


def _gpt2_block(dim):
    from afft_amd.models.future_prediction import GPT2Block
    return GPT2Block(dim, 4, 0.1, 0.1)


def _sa_fuser(dim):
    from afft_amd.models.fusion import ModalTokenCMFuser
    return ModalTokenCMFuser(dim, depth=1, num_heads=4, mlp_ratio=0.25, modalities={"rgb": dim, "flow": dim})


def _ca_fuser(dim):
    from afft_amd.models.fusion import TemporalCrossAttentFuser
    return TemporalCrossAttentFuser(dim, modalities={"rgb": dim, "flow": dim}, num_heads=4, mlp_ratio=0.25)


def _mapping(dim):
    from afft_amd.models.feature_mapping import Linear
    return Linear(64, dim, use_layernorm=True)


BUILDERS = [_block, _decoder_block, _gpt2_block, _sa_fuser, _ca_fuser, _mapping]


@pytest.mark.parametrize("build", BUILDERS, ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("width", [4160, 8192, 1026])
def test_unbuilt_layernorm_width_is_refused_at_construction(build, width):
    with pytest.raises(ValueError) as e:
        build(width)
    assert str(width) in str(e.value) and "4096" in str(e.value), str(e.value)


@pytest.mark.parametrize("build", [_block, _gpt2_block, _mapping], ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("width", [64, 2048, 2560, 4096])
def test_built_layernorm_widths_construct(build, width):
    with torch.device("meta"):      # no storage: only the constructor's checks are of interest
        m = build(width)
    norms = [mod for mod in m.modules() if isinstance(mod, torch.nn.LayerNorm)]
    assert norms and all(n.normalized_shape == (width,) for n in norms)


@pytest.mark.parametrize("build", [_sa_fuser, _ca_fuser], ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("width", [64, 2048, 2560, 4096])
def test_built_fuser_widths_construct(build, width):
    m = build(width)
    assert m.norm.normalized_shape == (width,)


def test_helper_takes_every_multiple_of_4_up_to_the_limit():
    from afft_amd import functional as F_
    assert F_.LN_MAX_WIDTH == 4096
    for w in (4, 64, 352, 2048, 2052, 4096):
        F_.check_ln_width(w, "test")
    for w in (2, 4097, 4100):
        with pytest.raises(ValueError):
            F_.check_ln_width(w, "test")
