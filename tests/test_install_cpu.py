"""Build-container tests of the drop-in claim: after afft_amd.install_as_models() the reference's import paths and Hydra
`_target_` strings resolve to this package, and every combination of the model configurations the reference ships
(conf/model: fuser, mapping, CMFP) instantiates through those paths, built by afft_amd.config.make_model_cfg with the
reference's `_target_` strings and keyword arguments."""
import importlib
import itertools
import sys

import pytest
import torch


@pytest.fixture()
def installed():
    saved = {k: v for k, v in sys.modules.items() if k == "models" or k.startswith("models.") or k == "common" or k.startswith("common.")}
    for k in saved:
        del sys.modules[k]
    import afft_amd
    afft_amd.install_as_models()
    yield afft_amd
    for k in [k for k in sys.modules if k == "models" or k.startswith("models.") or k == "common" or k.startswith("common.")]:
        del sys.modules[k]
    sys.modules.update(saved)


def test_reference_import_paths_resolve_here(installed):
    import afft_amd.models.fusion as ours
    assert importlib.import_module("models.fusion") is ours
    for name in ("base_model", "fusion", "transformerblock", "future_prediction", "feature_mapping"):
        assert importlib.import_module(f"models.{name}").__name__ == f"afft_amd.models.{name}"
    # registered whether or not `common` had been imported before the call
    for name in ("runner", "mixup", "transforms"):
        assert importlib.import_module(f"common.{name}").__name__ == f"afft_amd.common.{name}"
    from models.fusion import ModalTokenCMFuser, TemporalCrossAttentFuser   # noqa: F401
    from models.future_prediction import BaseFuturePredictor, CMFPEarly     # noqa: F401
    from common.runner import Runner                                        # noqa: F401


# The reference's conf/model choices, by file name, and the names afft_amd.config.make_model_cfg gives the same configurations
# (its restatement of common.yaml + fuser/*, mapping/*, future_predictor/*, CMFP/* with the same `_target_` strings and values)
FUSERS = {"SA-Fuser": "sa", "CA-Fuser": "ca", "SA-Fuser_wo_token": "cm", "T-SA-Fuser": "tsa", "MATT": "matt"}
MAPPINGS = {"linear": "linear", "gatedlinear": "gated", "nonlinear": "nonlinear"}
CMFPS = {"cmfp_early": "early", "scorefusion": "score", "individual": "individual"}

COMBOS = [(f, m, "cmfp_early") for f, m in itertools.product(["SA-Fuser", "CA-Fuser", "SA-Fuser_wo_token", "T-SA-Fuser"],
                                                               ["linear", "gatedlinear", "nonlinear"])] + \
         [("MATT", "linear", "scorefusion"), ("SA-Fuser", "linear", "individual")]


@pytest.mark.parametrize("fuser,mapping,cmfp", COMBOS)
def test_reference_yaml_configs_instantiate(installed, fuser, mapping, cmfp):
    from afft_amd.config import make_model_cfg
    modal_dims = {"rgb": 64, "objects": 24, "audio": 64, "flow": 64}
    late = cmfp != "cmfp_early"
    # the yaml's own values where make_model_cfg defaults to the bench's: no shared predictor, LayerNorm in the gated / non-linear mapping
    cfg = make_model_cfg(modal_dims, 64, 128, fuser=FUSERS[fuser], fp_layers=2, fp_heads=2, dropout=0.2, T=4,
                         modal_encoding=(fuser == "T-SA-Fuser"), cmfp=CMFPS[cmfp], mapping=MAPPINGS[mapping],
                         mapping_layernorm=(mapping != "linear"), share_predictors=False, share_classifiers=not late)
    if fuser == "T-SA-Fuser":
        cfg.fuser["temporal_sequence_length"] = 4
    for section in ("fuser", "mapping", "future_predictor", "CMFP"):
        assert cfg[section]["_target_"].startswith("models."), section
    from models.base_model import BaseModel        # the reference's import path (train.py:22)
    net = BaseModel(cfg, num_classes={"action": 11}, class_mappings={})
    assert type(net).__module__ == "afft_amd.models.base_model"
    names = [k for k, _ in net.named_parameters()]
    assert any(k.startswith("future_predictor.") for k in names)
    if not late:
        assert any(".fuser." in k for k in names)
        target = cfg.fuser["_target_"].rsplit(".", 1)[1]
        assert type(net.future_predictor.fuser).__name__ == target
