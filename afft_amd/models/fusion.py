"""MI355X mirror of the reference's ``models/fusion.py``:

  ModalTokenCMFuser         (SA-Fuser with modality token)   <- models/fusion.py:273-365
  TemporalCrossAttentFuser  (CA-Fuser)                       <- models/fusion.py:218-270
  CMFuser                   (SA-Fuser without the token)     <- models/fusion.py:61-118
  TemporalCMFuser           (T-SA-Fuser)                     <- models/fusion.py:121-215
  MATT                      (RULSTM modality attention)      <- models/fusion.py:35-58

Same constructor keywords (the Hydra surface of conf/model/fuser/{SA,CA}-Fuser.yaml), same parameter
names (checkpoints load unchanged), same return values.  Token assembly, the transformer blocks and the
final LayerNorm (on token 0 only: the reference normalises all S tokens and keeps one) run in HIP kernels.
"""
from __future__ import annotations

from typing import Callable, Dict, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from .. import dropout as D_
from .. import functional as F_
from .. import runtime as rt
from .transformerblock import Block, DecoderBlock


def trunc_normal_(t: Tensor, std: float = 0.02):
    return nn.init.trunc_normal_(t, std=std)


def _init_weights(m):
    # timm VisionTransformer style init used by the reference (models/fusion.py:21-27)
    if isinstance(m, nn.Linear):
        trunc_normal_(m.weight, std=.02)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)


def generate_square_subsequent_mask(sz: int):
    return torch.triu(torch.full((sz, sz), float('-inf')), diagonal=1)


def _check_same_shape(modal_feats: Dict[str, Tensor]):
    shape = next(iter(modal_feats.values())).shape
    assert all([v.shape == shape for v in modal_feats.values()]), \
        'The shape of all inputs of the fusion module should be the same!'
    return shape


def _rows(f: Tensor, BT: int, C: int) -> Tensor:
    f2 = f.reshape(BT, C)
    return f2 if f2.dtype == torch.float32 else f2.float()


class MATT(nn.Module):
    """modality attention module from RULSTM, an MLP with 3 layers (models/fusion.py:35-58): Linear-ReLU-Dropout twice,
    a Linear to one score per modality, softmax.  The ReLU and the (train-mode) dropout run in the GEMM epilogues."""

    def __init__(self, modal_dims, dim=None, drop_rate=0.8):
        super().__init__()
        num_modality = len(modal_dims)
        in_size = dim * num_modality if dim else sum(modal_dims.values())
        self.matt = nn.Sequential(nn.Linear(in_size, int(in_size / 4)), nn.ReLU(), nn.Dropout(drop_rate),
                                  nn.Linear(int(in_size / 4), int(in_size / 8)), nn.ReLU(), nn.Dropout(drop_rate),
                                  nn.Linear(int(in_size / 8), num_modality))

    def forward(self, modal_feats: Dict[str, Tensor], ordered_feature_list: Callable) -> Tensor:
        feats = torch.cat(ordered_feature_list(modal_feats), dim=2)
        B, Tn, C = feats.shape
        x = feats.reshape(B * Tn, C)
        x = x if x.dtype == torch.float32 else x.float()
        for i in (0, 3):
            lin, drop = self.matt[i], self.matt[i + 2]
            desc = D_.elementwise(drop.p) if (self.training and drop.p > 0) else None
            x = F_.LinearAct.apply(x, lin.weight, lin.bias, "relu", None, desc)
        lin = self.matt[6]
        x = F_.LinearAct.apply(x, lin.weight, lin.bias, "none", None, None)
        return F_.SoftmaxSmall.apply(x).view(B, Tn, -1)


class ModalTokenCMFuser(nn.Module):
    """Corresponds to SA-Fuser with modality token in the paper"""

    def __init__(self, dim, depth=1, num_heads=4, mlp_ratio=4., qkv_bias=False, qk_scale=None, embd_drop_rate=0.,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0., act_layer=nn.GELU,
                 norm_elementwise=True, cross_attn=False, modalities=None, modal_encoding=False,
                 frame_level_token=False, temporal_sequence_length=None):
        super().__init__()
        from functools import partial
        norm_layer = partial(nn.LayerNorm, eps=1e-6, elementwise_affine=norm_elementwise)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]  # stochastic depth decay rule
        self.blocks = nn.ModuleList([
            Block(dim=dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                  drop=drop_rate, attn_drop=attn_drop_rate, drop_path=dpr[i], act_layer=act_layer,
                  norm_layer=norm_layer) for i in range(depth)])
        F_.check_ln_width(dim, type(self).__name__)
        self.norm = norm_layer(dim)
        self.num_mods = len(modalities) + 1  # + the modality-agnostic token
        self.modality_embedding = nn.Parameter(torch.zeros(1, self.num_mods, dim)) if modal_encoding else None
        self.embd_drop = nn.Dropout(embd_drop_rate)
        self.cross_attn = cross_attn
        self.frame_level_token = frame_level_token
        self.temporal_sequence_length = temporal_sequence_length
        if not frame_level_token:
            self.modal_token = nn.Parameter(torch.zeros(1, 1, dim))
        else:
            assert temporal_sequence_length is not None, "Temporal sequence length must be provided!"
            self.modal_token = nn.Parameter(torch.zeros(1, temporal_sequence_length, dim))
        trunc_normal_(self.modal_token, std=.02)
        if self.modality_embedding is not None:
            trunc_normal_(self.modality_embedding, std=.02)
        self.apply(_init_weights)

    @staticmethod
    def generate_cross_attention_mask(sz):
        mask = torch.eye(sz)
        return mask.masked_fill(mask == 1, float('-inf'))

    def forward(self, modal_feats: Dict[str, Tensor], ordered_feature_list: Callable) -> Tuple[Tensor, Tensor]:
        B, T, C = _check_same_shape(modal_feats)
        feats = ordered_feature_list(modal_feats)
        S = len(feats) + 1
        if self.frame_level_token:
            assert self.temporal_sequence_length == T, \
                f"Temporal sequence length not valid {self.temporal_sequence_length} vs {T}"
        BT = B * T
        X = F_.AssembleTokens.apply(self.modal_token, self.modality_embedding, T, self.frame_level_token,
                                    *[_rows(f, BT, C) for f in feats])          # [BT*S, C]
        if self.training and self.embd_drop.p > 0:
            X = F_.ElementDropout.apply(X, D_.elementwise(self.embd_drop.p))
        mask = "diag" if self.cross_attn else "none"
        # the attention maps of all blocks in ONE buffer (the reference stacks the per-block tensors, models/fusion.py:366): every
        # block's kernel writes its slice, the stacked result is a view
        depth = len(self.blocks)
        maps = (torch.empty(depth, BT, self.blocks[0].attn.num_heads, S, S, dtype=torch.float32, device=X.device)
                if depth and X.is_cuda else None)      # (CPU test doubles write with in-place torch ops: version counters)
        attn_weights = []
        # Only token 0 of the last block's output is used (models/fusion.py:362-365): that block runs its MLP half on the
        # token-0 rows alone (Block.forward_rows_first_token) -- 4/5 of one block's MLP, 7 % of the step's FLOPs at M = 4,
        # that the reference computes and discards; every output and every gradient is unchanged.
        dead_rows = rt.skip_dead_rows()
        for i, blk in enumerate(self.blocks):
            po = maps[i] if maps is not None else None
            if dead_rows and i + 1 == len(self.blocks):
                X, probs = blk.forward_rows_first_token(X, S, mask, po)            # X [BT, C]
            else:
                X, probs = blk.forward_rows(X, S, mask, po)                        # probs [BT, H, S, S]
            attn_weights.append(probs.view(B, T, *probs.shape[1:]))
        z = F_.LayerNormRows.apply(X, self.norm.weight, self.norm.bias, self.norm.eps,
                                   1 if dead_rows and len(self.blocks) > 0 else S)  # token 0 of each frame
        stacked = maps.view(depth, B, T, *maps.shape[2:]) if maps is not None else torch.stack(attn_weights)
        return z.view(B, T, C), stacked.transpose(0, 1)


class CMFuser(nn.Module):
    """Corresponds to SA-Fuser without modality token in the paper (models/fusion.py:61-118): the M modality features
    of a frame attend to each other, the fused feature is the MEAN of the M output tokens."""

    def __init__(self, dim, depth=1, num_heads=4, mlp_ratio=4., qkv_bias=False, qk_scale=None, embd_drop_rate=0.,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0., act_layer=nn.GELU, norm_layer=None,
                 cross_attn=False):
        super().__init__()
        from functools import partial
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]  # stochastic depth decay rule
        self.blocks = nn.ModuleList([
            Block(dim=dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                  drop=drop_rate, attn_drop=attn_drop_rate, drop_path=dpr[i], act_layer=act_layer,
                  norm_layer=norm_layer) for i in range(depth)])
        F_.check_ln_width(dim, type(self).__name__)
        self.norm = norm_layer(dim)
        self.embd_drop = nn.Dropout(embd_drop_rate)
        self.cross_attn = cross_attn
        self.apply(_init_weights)

    @staticmethod
    def generate_cross_attention_mask(sz):
        mask = torch.eye(sz)
        return mask.masked_fill(mask == 1, float('-inf'))

    def forward(self, modal_feats: Dict[str, Tensor], ordered_feature_list: Callable) -> Tuple[Tensor, Tensor]:
        B, T, C = _check_same_shape(modal_feats)
        feats = ordered_feature_list(modal_feats)
        S = len(feats)
        BT = B * T
        X = F_.ScatterTokens.apply(*[_rows(f, BT, C) for f in feats]).view(BT * S, C)     # n * (B,T,C) -> (B*T, n, C)
        if self.training and self.embd_drop.p > 0:
            X = F_.ElementDropout.apply(X, D_.elementwise(self.embd_drop.p))
        mask = "diag" if self.cross_attn else "none"
        attn_weights = []
        for blk in self.blocks:
            X, probs = blk.forward_rows(X, S, mask)
            attn_weights.append(probs.view(B, T, *probs.shape[1:]))
        X = F_.LayerNormRows.apply(X, self.norm.weight, self.norm.bias, self.norm.eps, 1)
        z = F_.GroupMean.apply(X, BT, S, C)                                                # torch.mean(x, dim=1)
        return z.view(-1, T, C), torch.stack(attn_weights).transpose(0, 1)


class TemporalCMFuser(nn.Module):
    """Corresponds to T-SA-Fuser in the paper (models/fusion.py:121-215): temporal (causal) and multi-modal attention
    at the same time -- one sequence of num_mods * T tokens per clip, modality-major, under the causal T x T mask tiled
    over the modalities; frame position + modality embeddings."""

    def __init__(self, dim, depth=1, num_heads=4, mlp_ratio=4., qkv_bias=False, qk_scale=None, embd_drop_rate=0.,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0., act_layer=nn.GELU, norm_layer=None,
                 modalities=None, modal_encoding=True, frame_level_token=False, temporal_sequence_length=None,
                 max_position_embeddings=64):
        super().__init__()
        from functools import partial
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]  # stochastic depth decay rule
        self.blocks = nn.ModuleList([
            Block(dim=dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                  drop=drop_rate, attn_drop=attn_drop_rate, drop_path=dpr[i], act_layer=act_layer,
                  norm_layer=norm_layer) for i in range(depth)])
        F_.check_ln_width(dim, type(self).__name__)
        self.norm = norm_layer(dim)
        # frame position embedding and modality embedding
        self.num_mods = len(modalities) + 1 if frame_level_token else len(modalities)
        self.modality_embedding = nn.Parameter(torch.zeros(self.num_mods, dim)) if modal_encoding else None
        self.position_embeddings = nn.Embedding(max_position_embeddings, dim)
        self.position_embeddings.weight._afft_fp32_table = True      # fp32 rows for AddRowTable (parallel.FlatParams.owns_image)
        self.embd_drop = nn.Dropout(embd_drop_rate)
        self.frame_level_token = frame_level_token
        self.temporal_sequence_length = temporal_sequence_length
        self.modal_token = None        # modality agnostic token
        if frame_level_token:
            assert temporal_sequence_length is not None, "Temporal sequence length must be provided!"
            self.modal_token = nn.Parameter(torch.zeros(1, temporal_sequence_length, dim))
        if self.modal_token is not None:
            trunc_normal_(self.modal_token, std=.02)
        if self.modality_embedding is not None:
            trunc_normal_(self.modality_embedding, std=.02)
        self.apply(_init_weights)

    def forward(self, modal_feats: Dict[str, Tensor], ordered_feature_list: Callable) -> Tuple[Tensor, Tensor]:
        B, T, C = _check_same_shape(modal_feats)
        n = self.num_mods
        L = n * T
        if L > 512:
            raise NotImplementedError(f"afft_amd: T-SA-Fuser sequences of {L} tokens (> 512) are not built")
        feats = [_rows(f, B, T * C) for f in ordered_feature_list(modal_feats)]           # each (B, T*C)
        if self.frame_level_token:
            assert self.temporal_sequence_length == T, \
                f"Temporal sequence length not valid {self.temporal_sequence_length} vs {T}"
            feats = [F_.SinkParam.apply(self.modal_token).reshape(1, T * C).expand(B, -1)] + feats
        X = F_.ScatterTokens.apply(*feats).view(B * L, C)                                   # (B, n*T, C), modality-major
        # position embedding of the frame + modality embedding: one [n*T, C] table added to every clip
        table = F_.SinkParam.apply(self.position_embeddings.weight)[:T].repeat(n, 1)
        if self.modality_embedding is not None:
            table = table + F_.SinkParam.apply(self.modality_embedding).repeat_interleave(T, dim=0)
        X = F_.AddRowTable.apply(X, table, L, 0)
        if self.training and self.embd_drop.p > 0:
            X = F_.ElementDropout.apply(X, D_.elementwise(self.embd_drop.p))
        attn_weights = []
        for blk in self.blocks:
            X, probs = blk.forward_rows(X, L, ("blockcausal", T))                          # probs [B, H, L, L]
            attn_weights.append(probs)
        X = F_.LayerNormRows.apply(X, self.norm.weight, self.norm.bias, self.norm.eps, 1)
        if self.frame_level_token:
            z = X.view(B, L, C)[:, :T, :]       # the outputs of the frame-level modal tokens
        else:
            z = F_.GroupMean.apply(X, B, n, T * C).view(B, T, C)    # mean over the modality tokens of each frame
        return z, torch.stack(attn_weights).transpose(0, 1)


class TemporalCrossAttentFuser(nn.Module):
    """Corresponds to CA-Fuser in the paper: rgb is the query stream, every other modality a memory;
    depth = number of modalities - 1."""

    def __init__(self, dim, modalities=None, num_heads=4, mlp_ratio=4., qkv_bias=False, qk_scale=None,
                 embd_drop_rate=0., drop_rate=0., attn_drop_rate=0., drop_path_rate=0., act_layer=nn.GELU,
                 norm_layer=None, max_position_embeddings=128):
        super().__init__()
        from functools import partial
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        depth = len(modalities) - 1
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]
        self.blocks = nn.ModuleList([
            DecoderBlock(dim=dim, mem_dim=None, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                         qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate, drop_path=dpr[i],
                         act_layer=act_layer, norm_layer=norm_layer) for i in range(depth)])
        F_.check_ln_width(dim, type(self).__name__)
        self.norm = norm_layer(dim)
        self.embd_drop = nn.Dropout(embd_drop_rate)
        self.position_embeddings = nn.Embedding(max_position_embeddings, dim)
        self.position_embeddings.weight._afft_fp32_table = True      # fp32 rows for AddRowTable (parallel.FlatParams.owns_image)
        self.apply(_init_weights)

    def forward(self, modal_feats: Dict[str, Tensor], ordered_feature_list: Callable) -> Tuple[Tensor, Tensor]:
        B, T, C = _check_same_shape(modal_feats)
        feats = ordered_feature_list(modal_feats)
        BT = B * T
        table = self.position_embeddings.weight
        streams = []
        for f in feats:
            s = F_.AddRowTable.apply(_rows(f, BT, C).contiguous(), table, T, 0)
            if self.training and self.embd_drop.p > 0:
                s = F_.ElementDropout.apply(s, D_.elementwise(self.embd_drop.p))
            streams.append(s)
        x, mems = streams[0], streams[1:]
        for i, blk in enumerate(self.blocks):
            x = blk.forward_rows(x, mems[i], T, "causal")
        x = F_.LayerNormRows.apply(x, self.norm.weight, self.norm.bias, self.norm.eps, 1)
        dummy_attention = torch.zeros(B, requires_grad=False)  # to satisfy the framework (models/fusion.py:269)
        return x.view(B, T, C), dummy_attention
