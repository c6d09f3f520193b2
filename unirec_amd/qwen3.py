"""Qwen3 decoder + LoRA on the MI355X: the third-party half of the joint path.

The reference loads ``AutoModel.from_pretrained("Qwen/Qwen3-Embedding-0.6B")`` and wraps it with
``peft.get_peft_model`` (training/train_item_individual_token_joint.py:98-132); neither package's
source is part of the reference tree, so this module restates the published arithmetic
(transformers ``modeling_qwen3.py``: RMSNorm :59-64, MLP :81-83, RoPE :107-170, attention :185-280,
decoder layer :306-331, model :367-425) and the LoRA definition
``y = W x + (alpha/r) B A x`` with HF-compatible parameter names:
    embed_tokens.weight, layers.{i}.input_layernorm.weight, layers.{i}.self_attn.{q,k,v,o}_proj.weight,
    layers.{i}.self_attn.{q,k}_norm.weight, layers.{i}.post_attention_layernorm.weight,
    layers.{i}.mlp.{gate,up,down}_proj.weight, norm.weight
LoRA tensors are ``<proj>.lora_A.weight [r,in]`` / ``<proj>.lora_B.weight [out,r]`` (the only trainable
tensors, bias none: :123-129); ``peft_state_dict()`` exports them under peft's adapter key names.

Execution: the whole stack (embed + Q-Former token injection, 28 decoder layers, final norm, mean
pool over ALL positions :179-181) is ONE autograd node.  Base weights are frozen, so the backward is
dX GEMMs on the frozen bf16 weights plus rank-r reductions for dA/dB; every LoRA B-product rides in
the base GEMM's accumulators (second K-range of ur_gemm).  Activations are kept in HBM (288 GB:
no gradient checkpointing); only the RMSNorm outputs are recomputed in the backward.
"""
import contextlib
import math
from collections import namedtuple
from dataclasses import dataclass

import torch
import torch.nn as nn

from . import hip
from .packing import ParamPack, norm_device
from .switches import switches

BF16, F32 = torch.bfloat16, torch.float32
LORA_TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
# How the final hidden states become one vector per sequence.  "mean": over ALL S positions, padding included (the reference's rule, the
# default); "masked_mean": over the positions the attention mask marks valid; "last": the last valid position (last-token pooling, for
# either padding side).  The two mask-aware rules give embeddings that do not depend on the padded length.
POOLINGS = ("mean", "masked_mean", "last")


def normalize_pooling(value):
    """A pooling rule out of POOLINGS, or a ValueError that names the field."""
    if value not in POOLINGS:
        raise ValueError(f"pooling = {value!r} is not supported: one of {', '.join(POOLINGS)} is expected")
    return value


class Qwen3Config:
    """Shape of Qwen3-Embedding-0.6B by default (public model card)."""

    def __init__(self, vocab_size=151669, hidden_size=1024, intermediate_size=3072, num_hidden_layers=28,
                 num_attention_heads=16, num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-6, rope_theta=1e6,
                 lora_r=16, lora_alpha=32.0, lora_dropout=0.1, initializer_range=0.02,
                 lora_target_modules=None, lora_layers_to_transform=None, use_rslora=False, pooling="mean"):
        self.vocab_size, self.hidden_size, self.intermediate_size = vocab_size, hidden_size, intermediate_size
        self.num_hidden_layers, self.num_attention_heads, self.num_key_value_heads = num_hidden_layers, num_attention_heads, num_key_value_heads
        self.head_dim, self.rms_norm_eps, self.rope_theta = head_dim, rms_norm_eps, rope_theta
        self.lora_r, self.lora_alpha, self.lora_dropout = lora_r, lora_alpha, lora_dropout
        self.initializer_range = initializer_range
        # LoRA placement (peft's target_modules / layers_to_transform; None = all seven projections / every layer) and peft's
        # use_rslora (scale lora_alpha / sqrt(r) instead of lora_alpha / r)
        self.lora_target_modules, self.lora_layers_to_transform, self.use_rslora = lora_target_modules, lora_layers_to_transform, bool(use_rslora)
        self.pooling = normalize_pooling(pooling)


def normalize_lora_targets(spec):
    """peft's ``target_modules`` -> the projections that carry an adapter, as a tuple of names out of LORA_TARGETS in that order.
    None and "all-linear" mean all seven; a list / tuple / set holds plain (``q_proj``) or dotted (``self_attn.q_proj``) names.
    Anything peft would reject (an empty collection, a name that matches no projection) and what this package does not take
    (a regular expression, i.e. any other string) raises ValueError."""
    if spec is None:
        return LORA_TARGETS
    if isinstance(spec, str):
        if spec == "all-linear":
            return LORA_TARGETS
        raise ValueError(f"target_modules = {spec!r}: a string is a peft regular expression, which is not supported; pass a list of names out of "
                         f"{', '.join(LORA_TARGETS)} (or 'all-linear')")
    if not isinstance(spec, (list, tuple, set, frozenset)):
        raise ValueError(f"target_modules must be a list, tuple or set of projection names, got {type(spec).__name__}")
    dotted = {p.rsplit(".", 1)[-1]: p for _, projs in ADAPTER_GROUPS for p in projs}
    chosen = set()
    for name in spec:
        short = str(name).rsplit(".", 1)[-1]
        if short not in dotted or str(name) not in (short, dotted[short]):
            raise ValueError(f"target_modules: {name!r} matches no projection of the decoder ({', '.join(LORA_TARGETS)})")
        chosen.add(short)
    if not chosen:
        raise ValueError("target_modules is empty: no projection would carry an adapter")
    return tuple(t for t in LORA_TARGETS if t in chosen)


def normalize_lora_layers(spec, num_layers):
    """peft's ``layers_to_transform`` -> the ascending tuple of layer indices that carry adapters.  None: every layer; an int or a list
    of ints in [0, num_layers); anything else raises ValueError."""
    if spec is None:
        return tuple(range(num_layers))
    items = [spec] if isinstance(spec, int) else (list(spec) if isinstance(spec, (list, tuple, set, frozenset)) else None)
    if not items or any(isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < num_layers for i in items):
        raise ValueError(f"layers_to_transform = {spec!r}: an int or a non-empty list of ints in [0, {num_layers}) is expected")
    return tuple(sorted(set(items)))


class _Proj(nn.Module):
    def __init__(self, fin, fout, r):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(fout, fin), requires_grad=False)
        if r > 0:
            self.lora_A = nn.Linear(fin, r, bias=False)
            self.lora_B = nn.Linear(r, fout, bias=False)


class _Norm(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d), requires_grad=False)


class _Attn(nn.Module):
    def __init__(self, c, r, on):
        super().__init__()
        D, hd = c.hidden_size, c.head_dim
        self.q_proj = _Proj(D, c.num_attention_heads * hd, r if "q_proj" in on else 0)
        self.k_proj = _Proj(D, c.num_key_value_heads * hd, r if "k_proj" in on else 0)
        self.v_proj = _Proj(D, c.num_key_value_heads * hd, r if "v_proj" in on else 0)
        self.o_proj = _Proj(c.num_attention_heads * hd, D, r if "o_proj" in on else 0)
        self.q_norm = _Norm(hd)
        self.k_norm = _Norm(hd)


class _MLP(nn.Module):
    def __init__(self, c, r, on):
        super().__init__()
        self.gate_proj = _Proj(c.hidden_size, c.intermediate_size, r if "gate_proj" in on else 0)
        self.up_proj = _Proj(c.hidden_size, c.intermediate_size, r if "up_proj" in on else 0)
        self.down_proj = _Proj(c.intermediate_size, c.hidden_size, r if "down_proj" in on else 0)


class _Layer(nn.Module):
    def __init__(self, c, r, on=LORA_TARGETS):
        """on: the projections of this layer that carry an adapter (names out of LORA_TARGETS); the others are built with r = 0"""
        super().__init__()
        self.self_attn = _Attn(c, r, on)
        self.mlp = _MLP(c, r, on)
        self.input_layernorm = _Norm(c.hidden_size)
        self.post_attention_layernorm = _Norm(c.hidden_size)


class _TokenTable(nn.Module):
    def __init__(self, v, d):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(v, d), requires_grad=False)


# The four adapter groups of a layer: the adapters of a group read the same input, so they share one set of dropout-bit planes, one
# down-projection launch and one A^T.  (key of the group's t / bits entries in saved["layers"][i], its projections)
ADAPTER_GROUPS = (("qkv", ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj")), ("o", ("self_attn.o_proj",)),
                  ("gu", ("mlp.gate_proj", "mlp.up_proj")), ("d", ("mlp.down_proj",)))
# What the persistent GEMM takes as a LoRA second K range: ONE K tile (csrc/gemm.hip, pers_takes: K2 <= BK = 64).  The one host-side
# statement of that constant; tests/test_gemm_plan.py holds it to the library's answer (hip.gemm_plan).
PERS_GEMM_K2_MAX = 64
_MAX_SHARED_ADAPTERS = max(len(projs) for _, projs in ADAPTER_GROUPS)      # q|k|v: the widest merged launch


def lora_rank_rule(r, sw=switches, adapters=None):
    """The launch choices that depend on the LoRA rank: a pure function of (rank, switches, placement), read by Qwen3LoRAModel._plan.
    adapters: the most adapters any q|k|v or gate|up group of the model holds (None: all three of q|k|v).
      merged      q|k|v and gate|up leave as one launch each while the merged launch's second K range (adapters * r) still fits the
                  persistent GEMM; otherwise one launch per projection (K2 = r <= 64 each)
      fuse_norm   RMSNorm + down projection as one kernel (ur_rmsnorm_lora_fwd: rank 16)
      swiglu_lora SwiGLU + the down adapter's down projection as one kernel (ur_swiglu_lora_fwd: rank 16)
      bits_t      token-packed dropout flags: only the rank-16 ring kernel of ur_lora_reduce consumes them"""
    r = int(r)
    nad = _MAX_SHARED_ADAPTERS if adapters is None else int(adapters)
    return {"merged": bool(sw.merge_proj) and nad * r <= PERS_GEMM_K2_MAX,
            "fuse_norm": bool(sw.fuse_norm_lora) and r == 16,
            "swiglu_lora": bool(sw.fuse_swiglu_lora) and r == 16,
            "bits_t": bool(sw.bits_t) and r == 16}


def lora_bits_t_sizes(M=None, W=None):
    """Token-packed flags are made only where ur_lora_reduce's ring kernel consumes them: M tokens in whole 128-token tiles, an adapter
    input of W columns in whole 64-column pieces (a size left out is not asked about).  tests/test_lora_plan.py holds this and
    lora_rank_rule's bits_t to the library's own selection (hip.lora_plan)."""
    return (M is None or M % 128 == 0) and (W is None or W % 64 == 0)


_QK_FUSE_MAX_RATIO = 4.0      # largest |w_d| / |w_{d+64}| spread of a rotate-half pair of the q / k norm weights under which the fused epilogue is used


# parameter names of one adapter group of one layer: a = the lora_A.weight of every adapter (the tuple is also the key of the group's A^T
# in _lora_transposes), b = the lora_B.weight of every adapter
_GroupNames = namedtuple("_GroupNames", "a b")
# where the PRESENT adapters of one adapter group of one layer sit (built once, beside the names):
#   planes  dropout bit planes to generate: the group's planes 0 .. highest present slot (a module's slot is its position in the
#           ADAPTER_GROUPS entry, whatever else is present: its mask never depends on the placement); 0 = no adapter
#   view    the slice of those planes that holds the present adapters' (every subset of three slots is an arithmetic progression: the
#           kernels take a base + plane stride); None = all of them, the tensor itself
#   cols    (first column, width) of every present adapter inside the group's merged output
#   split   the group as one launch per projection: (first output column, width, index of the adapter among the present ones or None,
#           its lora_B name or None) for EVERY projection of the group
_GroupPlace = namedtuple("_GroupPlace", "planes view cols split")


@dataclass(frozen=True)
class _Plan:
    """The launch choices of one forward: constant over its layers, taken once before the loop (Qwen3LoRAModel._plan) and kept in
    saved["plan"], where the backward reads what the forward did.  It describes the layers that carry adapters; a group without an
    adapter (a layer outside layers_to_transform, a group nobody targets) runs as the adapter-free model runs it: one launch, no down
    projection, and of the fused forms those the plan queried for a launch without a second K range (fuse_rope, "pair")."""
    merged: bool            # q|k|v and gate|up leave as one launch each (always so without adapters), not one per projection
    fuse_norm: bool         # RMSNorm + the q|k|v / gate|up adapters' down projection as one kernel
    fuse_rope: bool         # q/k-norm + RoPE in the q|k|v launch's epilogue: no raw q, k exist
    swiglu: str             # "pair": epilogue of the merged gate|up launch, "up": epilogue of the up projection's own launch,
    #                         "lora": one pass with the down adapter's down projection (swiglu_lora_fwd), "alone": its own pass
    pad_att: bool           # attention output rows padded by 64 columns
    bits_one_event: bool    # wait for every layer's prefetched planes before the first layer
    mlp_recompute: str      # under recompute_mlp: the launch that rebuilds gate|up and act, "pair" / "merged" / "plain" (no adapters); None
    #                         (the per-adapter launches): the layer keeps them
    rope_bwd_in_dq: bool    # backward: the q heads' q/k-norm + RoPE backward rides in the dQ kernel's store ...
    rope_k_in_dkv: bool     # ... and the k heads' in the dK/dV kernel's (from the roped outputs only)
    bits_t: bool            # backward: token-packed dropout flags for the token reductions that have no prefetched copy


class _JointFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, item_tokens16, input_ids, mask_u8, first_special_id, anchor):
        pooled, saved = model._forward_impl(item_tokens16, input_ids, mask_u8, first_special_id)
        ctx.model, ctx.saved = model, saved
        return pooled

    @staticmethod
    def backward(ctx, d_pooled):
        d_tok = ctx.model._backward_impl(ctx.saved, d_pooled)
        ctx.saved = None
        return None, d_tok, None, None, None, None


class Qwen3LoRAModel(nn.Module):
    """Frozen Qwen3 decoder with LoRA adapters on the projections and layers the config names (default: all 7, every layer)."""

    def __init__(self, config: Qwen3Config, use_lora=True):
        super().__init__()
        self.config = config
        self.pooling = normalize_pooling(getattr(config, "pooling", "mean"))      # (a config object from before the field: the default)
        r = config.lora_r if use_lora else 0
        self.use_lora = r > 0
        if self.use_lora and int(r) not in hip.LORA_RANKS:
            raise ValueError(f"Qwen3LoRAModel: lora_r = {r} is not supported; the adapter kernels are built for the ranks "
                             f"{', '.join(map(str, hip.LORA_RANKS))} (one rank for all modules: no rank_pattern)")
        self.embed_tokens = _TokenTable(config.vocab_size, config.hidden_size)
        targets = normalize_lora_targets(config.lora_target_modules) if self.use_lora else ()
        adapted = set(normalize_lora_layers(config.lora_layers_to_transform, config.num_hidden_layers)) if self.use_lora else set()
        on = [targets if i in adapted else () for i in range(config.num_hidden_layers)]
        # the placement: per layer, the dotted names of the projections that carry an adapter, in canonical order
        self.adapter_modules = tuple(tuple(p for _, projs in ADAPTER_GROUPS for p in projs if p.rsplit(".", 1)[-1] in on[i])
                                     for i in range(config.num_hidden_layers))
        self.layers = nn.ModuleList([_Layer(config, r, on[i]) for i in range(config.num_hidden_layers)])
        self.norm = _Norm(config.hidden_size)
        self._pack = None
        self._frozen = None
        self._merged = None            # merge_adapter(): {"key", "fz", "bytes"} -- bf16 operands built from W + s B A
        self._adapters_off = False     # inside disable_adapter()
        self._rope = None
        self.grad_ready_hook = None
        self.lora_seed = 0x5EED        # base seed of the LoRA dropout masks (per run; identical on every data-parallel rank)
        # index of this forward's first sequence in the GLOBAL minibatch = dp_rank * B (unirec_amd.dp.set_dp_rank) unless
        # sample_offset is given: masks are keyed on the global token row (first * S + local row), so a data-parallel rank
        # draws exactly the masks its sequences would get in a single-process run over the whole minibatch
        self.dp_rank = 0
        self.sample_offset = None
        self._lora_step = 0            # forward calls with dropout so far: every step draws new masks
        self._bcomb = None             # block-diagonal LoRA B operands of the merged q|k|v and gate|up launches
        self._bits_stream = None       # side stream + planes of prefetch_lora_bits
        self._bits_pre = None
        self.recompute_mlp = switches.recompute_mlp   # drop gate|up and act after the forward, rebuild them in the backward
        self.keep_norm_outputs = True   # keep the two RMSNorm outputs per layer for the backward (memory for time); False recomputes them
        self._index_adapters()
        self.reset_parameters()

    def _index_adapters(self):
        """The tables derived from adapter_modules (built once, and again when merge_and_unload() removes the adapters)."""
        config = self.config
        # [layer][adapter group] -> parameter names, built once: the hot loops format no strings
        # (the PRESENT adapters of the group: the tuples may be empty)
        self._names = [[_GroupNames(a=tuple(f"layers.{i}.{p}.lora_A.weight" for p in projs if p in mods),
                                    b=tuple(f"layers.{i}.{p}.lora_B.weight" for p in projs if p in mods))
                        for _, projs in ADAPTER_GROUPS] for i, mods in enumerate(self.adapter_modules)]
        self._place = [[self._group_place(i, g) for g in range(len(ADAPTER_GROUPS))] for i in range(config.num_hidden_layers)]
        # the adapter counts that occur in a q|k|v / gate|up group over the layers (a layer outside layers_to_transform counts 0): the second K
        # ranges the merged launches are asked about (_plan)
        self._nad_qkv, self._nad_gu = (sorted({len(nm[g].a) for nm in self._names}) for g in (0, 2))

    def reset_parameters(self, lora_b_std=0.0):
        """Base N(0, initializer_range) (weights are random: no network for the checkpoint); LoRA A
        kaiming-uniform(a=sqrt(5)), B zeros -- peft's default init.  lora_b_std > 0 draws B ~ N(0, std)
        so the LoRA path is numerically exercised."""
        std = self.config.initializer_range
        for n, p in self.named_parameters():
            if n.endswith("lora_A.weight"):
                nn.init.kaiming_uniform_(p, a=math.sqrt(5))
            elif n.endswith("lora_B.weight"):
                if lora_b_std > 0:
                    nn.init.normal_(p, std=lora_b_std)
                else:
                    nn.init.zeros_(p)
            elif n.endswith("norm.weight") or n.endswith("layernorm.weight"):
                nn.init.ones_(p)
            else:
                nn.init.normal_(p, std=std)

    def resize_token_embeddings(self, new_size):
        """train_item_individual_token_joint.py:112-119 (rows for the added special tokens)."""
        old = self.embed_tokens.weight.data
        if new_size == old.shape[0]:
            return
        new = torch.empty(new_size, old.shape[1], dtype=old.dtype, device=old.device).normal_(std=self.config.initializer_range)
        n = min(new_size, old.shape[0])
        new[:n] = old[:n]
        self.embed_tokens.weight = nn.Parameter(new, requires_grad=False)
        self.config.vocab_size = new_size
        self._frozen = None

    def load_base_weights(self, state_dict, strict=True):
        """Frozen base weights from a Qwen3Model / Qwen3-Embedding state_dict (HF key names, optional ``model.`` or
        ``base_model.model.`` prefix).  A checkpoint vocabulary smaller than the (resized) table fills the first rows and
        leaves the added special-token rows alone -- ``load_state_dict(strict=False)`` cannot do that: it raises on the
        shape mismatch.  LoRA tensors in the dict are loaded too.  strict: every base tensor must be present."""
        sd = {}
        for k, v in state_dict.items():
            for pre in ("base_model.model.", "model."):
                if k.startswith(pre):
                    k = k[len(pre):]
            sd[k] = v
        own = dict(self.named_parameters())
        missing, unexpected = [], [k for k in sd if k not in own and k != "lm_head.weight"]
        with torch.no_grad():
            for k, p in own.items():
                if k not in sd:
                    if ".lora_" not in k:
                        missing.append(k)
                    continue
                v = sd[k]
                if k == "embed_tokens.weight" and v.shape[0] != p.shape[0]:
                    if v.shape[0] > p.shape[0] or v.shape[1] != p.shape[1]:
                        raise RuntimeError(f"embed_tokens.weight: checkpoint {tuple(v.shape)} does not fit the table {tuple(p.shape)}")
                    p[:v.shape[0]].copy_(v.to(p.device, p.dtype))
                    continue
                if tuple(v.shape) != tuple(p.shape):
                    raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(v.shape)} vs model {tuple(p.shape)}")
                p.copy_(v.to(p.device, p.dtype))
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_base_weights: missing {missing[:5]}{'...' if len(missing) > 5 else ''}, unexpected {unexpected[:5]}")
        self._frozen = None
        if self._pack is not None:
            self._pack.mark_dirty()
        return missing, unexpected

    # ---- parameter plumbing ---------------------------------------------------------------------
    def lora_named_parameters(self):
        named = dict(self.named_parameters())
        # per layer: every A (group by group: the adapters of a group are neighbours in the pack, fused16 / fusedg), then every B
        return [(n, named[n]) for groups in self._names for ab in "ab" for g in groups for n in getattr(g, ab)]

    def _ensure_pack(self, device):
        if not self.use_lora:
            return None
        if self._pack is None or not self._pack.is_current() or self._pack.device != norm_device(device):
            self._pack = ParamPack(self.lora_named_parameters(), device)
        return self._pack

    @property
    def pack(self):
        return self._pack

    def _ensure_frozen(self, device):
        """bf16 operands of the frozen base weights, fused per layer: [q|k|v], o, [gate|up], down."""
        # keyed on EVERY frozen tensor (storage + in-place version): loading any of them after a forward has run must not
        # leave stale bf16 / transposed copies behind
        key = (str(device), switches.fuse_qk_rope, switches.fuse_swiglu_gemm) + tuple((p.data_ptr(), p._version) for n, p in self.named_parameters() if ".lora_" not in n)
        if self._frozen is not None and self._frozen["key"] == key:
            return self._frozen
        fz = {"key": key, "layers": []}
        dev = torch.device(device)

        def c16(t):
            return hip.cast_f32_to_bf16(t.detach().to(dev, F32).contiguous())
        fz["embed"] = c16(self.embed_tokens.weight)
        fz["norm"] = self.norm.weight.detach().to(dev, F32).contiguous()
        for lyr in self.layers:
            a, m = lyr.self_attn, lyr.mlp
            wqkv = torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], 0)
            wgu = torch.cat([m.gate_proj.weight, m.up_proj.weight], 0)
            rp = self._qk_row_perm(dev)
            fz["layers"].append({
                "qkv": c16(wqkv),
                # q|k|v with the rows of every q / k head in the paired order of the fused q/k-norm + RoPE epilogue (hip.qkrope_perm)
                # (only when that path can be selected at all: the duplicates cost ~0.6 GB at Qwen3-0.6B)
                "qkvP": c16(wqkv.to(dev)[rp]) if (rp is not None and switches.fuse_qk_rope) else None,
                # gate|up with 128-row blocks of gate and up interleaved (hip.swiglu_pair_rows): the paired SwiGLU forward epilogue
                "guP": c16(wgu.to(dev)[self._swiglu_rows(m.gate_proj.weight.shape[0], dev)]) if (switches.fuse_swiglu_gemm and m.gate_proj.weight.shape[0] % 128 == 0) else None,
                "o": c16(a.o_proj.weight), "gu": c16(wgu), "d": c16(m.down_proj.weight),
                # frozen => one-time transposed copies, so every dX GEMM is K-contiguous on both operands
                "qkvT": c16(wqkv.t()), "oT": c16(a.o_proj.weight.t()), "guT": c16(wgu.t()), "dT": c16(m.down_proj.weight.t()),
                "qn": a.q_norm.weight.detach().to(dev, F32).contiguous(), "kn": a.k_norm.weight.detach().to(dev, F32).contiguous(),
                "ln1": lyr.input_layernorm.weight.detach().to(dev, F32).contiguous(),
                "ln2": lyr.post_attention_layernorm.weight.detach().to(dev, F32).contiguous()})
        # The fused epilogue's backward recovers the normalised rows from the bf16 roped outputs (x^ = R^T(o) / w): the rounding
        # error of a rotate-half pair (d, d + 64) scales with the larger of its two entries and is divided by each one's own weight,
        # i.e. it is amplified by max(|w_d|, |w_{d+64}|) / min(...).  Fuse only while that conditioning stays small; a checkpoint
        # with widely spread norm weights takes the separate q/k-norm + RoPE pass (which keeps the raw q, k).
        def well_conditioned(w):
            a = w.abs().view(2, -1)
            lo, hi = torch.minimum(a[0], a[1]), torch.maximum(a[0], a[1])
            return bool((lo > 0).all()) and bool((hi <= _QK_FUSE_MAX_RATIO * lo).all())
        fz["qk_norm_fusable"] = all(well_conditioned(l["qn"]) and well_conditioned(l["kn"]) for l in fz["layers"])
        self._frozen = fz
        return fz

    def _swiglu_rows(self, I, device):
        """hip.swiglu_pair_rows(I) on `device`, built once (a host -> device copy per forward would block the host on the stream)"""
        key = (str(device), int(I))
        if getattr(self, "_sp", None) is None or self._sp[0] != key:
            self._sp = (key, hip.swiglu_pair_rows(I).to(device))
        return self._sp[1]

    def _qk_row_perm(self, device):
        """Row order of the paired q|k|v operand: inside every q / k head tile column c holds feature qkrope_perm[c]; v rows stay."""
        c = self.config
        if c.head_dim != 128:
            return None
        key = (str(device), c.num_attention_heads, c.num_key_value_heads)
        if getattr(self, "_rp", None) is None or self._rp[0] != key:
            perm = hip.qkrope_perm(128)
            nqk = c.num_attention_heads + c.num_key_value_heads
            rows = torch.cat([(torch.arange(nqk)[:, None] * 128 + perm[None, :]).reshape(-1),
                              torch.arange(nqk * 128, (nqk + c.num_key_value_heads) * 128)])
            self._rp = (key, rows.to(device))
        return self._rp[1]

    def _rope_tables(self, S, device):
        if self._rope is None or self._rope[0] != (S, str(device)):
            self._rope = ((S, str(device)), hip.rope_table(S, self.config.head_dim, float(self.config.rope_theta), device))
        return self._rope[1]

    def peft_state_dict(self):
        """LoRA tensors under peft's adapter key names (save_pretrained compatibility, :183-200)."""
        out = {}
        for n, p in self.named_parameters():
            if ".lora_A." in n or ".lora_B." in n:
                out["base_model.model." + n] = p.detach().cpu()
        return out

    # ---- merged adapters (peft's merge_adapter / unmerge_adapter / merge_and_unload / disable_adapter) ---------------------------
    @property
    def merged(self):
        return self._merged is not None

    def _lora_live(self):
        """adapters exist and the forward runs their streams: not merged, not inside disable_adapter()"""
        return self.use_lora and self._merged is None and not self._adapters_off

    def _adapted_projections(self):
        """(layer index, adapter group, first row and row count inside the group's fused operand, the _Proj) of every projection that
        carries an adapter"""
        for i, lyr in enumerate(self.layers):
            for g, (_, projs) in enumerate(ADAPTER_GROUPS):
                for (col, n, j, _), pname in zip(self._place[i][g].split, projs):
                    if j is not None:
                        yield i, g, col, n, lyr.get_submodule(pname)

    def refuse_training_while_merged(self):
        """A training forward on merged operands would train nothing (the adapter streams do not run) and silently drop LoRA dropout:
        refused, before any launch."""
        if self._merged is not None and self.training and torch.is_grad_enabled():
            raise RuntimeError("Qwen3LoRAModel: the adapters are merged into the frozen operands (merge_adapter()); a training forward "
                               "needs the adapter streams: call unmerge_adapter() first")

    def _ensure_merged(self, device):
        """The frozen operands with W + s B A in place of W for every projection that carries an adapter: every layout _ensure_frozen
        keeps (qkv, qkvP, gu, guP, o, d and the four transposes) is rebuilt from the merged bf16 values (ur_lora_merge from the f32 masters,
        one rounding to bf16); groups and layers without an adapter share the unmerged tensors.  Cached under a key that holds the base
        weights' state and the adapters' (storage, in-place version, the pack's generation: the fused optimizer writes the masters raw)."""
        base = self._ensure_frozen(device)
        s = self._lora_scale()
        key = (base["key"], s, tuple((n, p.data_ptr(), p._version) for n, p in self.lora_named_parameters()),
               None if self._pack is None else (id(self._pack), self._pack.generation))
        if self._merged is not None and self._merged["key"] == key:
            return self._merged["fz"]
        dev = torch.device(device)
        layers = [dict(fl) if self.adapter_modules[i] else fl for i, fl in enumerate(base["layers"])]
        fresh = {}      # (layer, group) -> the group's merged operand: a copy of the unmerged one, the adapted rows overwritten

        def f32(t):
            return t.detach().to(dev, F32).contiguous()
        for i, g, col, n, proj in self._adapted_projections():
            name = ADAPTER_GROUPS[g][0]
            if (i, g) not in fresh:
                fresh[(i, g)] = base["layers"][i][name].clone()
            hip.lora_merge(f32(proj.weight), f32(proj.lora_A.weight), f32(proj.lora_B.weight), s, out_bf16=fresh[(i, g)][col:col + n])
        nbytes = 0
        for (i, g), w16 in fresh.items():
            name, fl = ADAPTER_GROUPS[g][0], layers[i]
            fl[name], fl[name + "T"] = w16, w16.t().contiguous()
            if name == "qkv" and fl["qkvP"] is not None:
                fl["qkvP"] = w16[self._qk_row_perm(dev)]
            if name == "gu" and fl["guP"] is not None:
                fl["guP"] = w16[self._swiglu_rows(self.config.intermediate_size, dev)]
            nbytes += sum(fl[k].numel() * 2 for k in (name, name + "T", name + "P") if fl.get(k) is not None)
        fz = dict(base, layers=layers)
        self._merged = {"key": key, "fz": fz, "bytes": nbytes}
        return fz

    def merge_adapter(self, device=None):
        """peft's merge_adapter(): from now on every forward runs the adapter-free path on bf16 operands made of W + s B A (s =
        _lora_scale(): rsLoRA is honoured) -- no RMSNorm + adapter kernels, no lora_project, no second K range, no dropout planes.  The f32
        masters and the LoRA parameters are not touched.  Evaluation only: a training forward is refused until unmerge_adapter().
        device: where the operands are built (default: where the weights are)."""
        if not self.use_lora:
            return
        dev = norm_device(self.embed_tokens.weight.device if device is None else device)      # (indexed: the key a forward's inputs give)
        if dev.type != "cuda":
            raise hip._lib.UniRecHipError("merge_adapter: the merge runs on the MI355X only (no CPU fallback): move the model to the device first")
        self._release_prefetched(dev)
        self._ensure_merged(dev)

    def unmerge_adapter(self):
        """Drop the merged operands.  The next forward runs on the unmerged operands, which are (re)built from the untouched f32
        masters: exact, where peft subtracts s B A back out of the merged weight."""
        self._merged = None

    @contextlib.contextmanager
    def disable_adapter(self):
        """peft's disable_adapter(): inside the context the base model runs without adapters (the adapter-free path on the unmerged
        operands), merged or not; nothing is changed."""
        prev, self._adapters_off = self._adapters_off, True
        try:
            yield self
        finally:
            self._adapters_off = prev

    def _operands(self, device):
        """(frozen operands, parameter pack) of a forward: merged operands or disabled adapters run without the pack, which is what a
        model built with use_lora=False runs."""
        if self._adapters_off:
            return self._ensure_frozen(device), None
        if self._merged is not None:
            return self._ensure_merged(device), None      # (re-keyed: a weight or adapter loaded while merged rebuilds them)
        return self._ensure_frozen(device), self._ensure_pack(device)

    def merged_state_dict(self, dtype=F32):
        """The HF ``Qwen3Model`` state dict with the adapters folded in (W + s B A by ur_lora_merge into temporaries: the model is not
        modified), on the CPU in `dtype`.  After merge_and_unload() this is state_dict() itself."""
        adapted = {id(proj.weight): proj for _, _, _, _, proj in self._adapted_projections()}
        s, out = self._lora_scale(), {}
        for n, p in self.named_parameters():
            if ".lora_" in n:
                continue
            proj = adapted.get(id(p))
            w = p.detach() if proj is None else hip.lora_merge(p.detach().contiguous(), proj.lora_A.weight.detach().contiguous(),
                                                                proj.lora_B.weight.detach().contiguous(), s)[0]
            out[n] = w.to("cpu", dtype).contiguous()
        return out

    def merge_and_unload(self):
        """peft's merge_and_unload(): W <- W + s B A in place on the f32 masters of every projection that carries an adapter, then the
        adapters are removed: use_lora is False, state_dict() holds exactly the HF Qwen3Model keys.  Returns self."""
        if not self.use_lora:
            return self
        self._release_prefetched(self.embed_tokens.weight.device)
        s = self._lora_scale()      # (hip.lora_merge refuses host tensors: there is no CPU fallback of the merge)
        for _, _, _, _, proj in list(self._adapted_projections()):
            w = proj.weight.data
            hip.lora_merge(w, proj.lora_A.weight.detach().contiguous(), proj.lora_B.weight.detach().contiguous(), s, out_f32=w)
            del proj.lora_A, proj.lora_B
        self.use_lora = False
        self.adapter_modules = tuple(() for _ in self.layers)
        self._index_adapters()
        # (the kernel wrote the masters raw: no version counter moved, so the bf16 operands are dropped by hand)
        self._frozen = self._merged = self._pack = self._bcomb = self._lt = None
        return self

    # ---- public forward ---------------------------------------------------------------------------
    def forward_pooled(self, input_ids, attention_mask=None, item_tokens16=None, first_special_id=0):
        """input_ids int64 [B,S]; attention_mask [B,S] or None; item_tokens16 [B,T,D] bf16 (Q-Former
        query tokens to inject at ids first_special_id + t) or None -> pooled f32 [B,D] (self.pooling: the mean over all S positions
        by default; "masked_mean" / "last" look at attention_mask)."""
        self.refuse_training_while_merged()
        if not input_ids.is_cuda:
            raise hip._lib.UniRecHipError("Qwen3LoRAModel runs on the MI355X only (no CPU fallback in the product path)")
        B, S = input_ids.shape
        mask_u8 = None if attention_mask is None else (attention_mask != 0).to(torch.uint8).contiguous()
        if item_tokens16 is None:
            item_tokens16 = torch.zeros((B, 0, self.config.hidden_size), dtype=BF16, device=input_ids.device)
        # the LoRA gradients are side effects of this node's backward: an anchor input keeps the node
        # alive even when the injected tokens do not require grad (frozen / absent Q-Former)
        if not torch.is_grad_enabled():
            # inference (MRREvaluator, CatalogEvaluator, token caches): nothing is kept for a backward, so the peak is one
            # layer's activations instead of all of them (178 GB at B=64, S=2048 in training)
            return self._forward_impl(item_tokens16.detach(), input_ids.contiguous(), mask_u8, int(first_special_id), keep=False)[0]
        anchor = torch.zeros(1, device=input_ids.device, requires_grad=True) if self._lora_live() else None
        return _JointFn.apply(self, item_tokens16, input_ids.contiguous(), mask_u8, int(first_special_id), anchor)

    # ---- implementation ---------------------------------------------------------------------------
    def _drop_p(self):
        """peft applies lora_dropout only in training mode (nn.Dropout inside every LoraLayer)."""
        return float(self.config.lora_dropout) if (self.training and self._lora_live()) else 0.0

    def lora_dropout_seed(self, step, layer, group):
        """Seed of the dropout masks of one adapter group (the adapters that share an input: 0 = q|k|v, 1 = o,
        2 = gate|up, 3 = down) -- a pure function of (base seed, step, layer, group); tests regenerate the bit
        planes from it (hip.lora_dropout_bits) and feed the unpacked masks to the oracle."""
        # splitmix64 of the combined index: the seeds of neighbouring (step, layer, group) differ in every bit, not in a
        # few low ones (the mask streams of two adapter groups must be unrelated, as peft's per-module nn.Dropout are)
        z = (int(self.lora_seed) * 0x9E3779B97F4A7C15 + int(step) * 0xD1B54A32D192ED03 + (layer * 8 + group + 1) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return (z ^ (z >> 31)) & 0x7FFFFFFFFFFFFFFF

    def first_sample(self, B):
        return int(self.sample_offset) if self.sample_offset is not None else int(self.dp_rank) * int(B)

    def _group_dims(self):
        """(input width, output width of every adapter) of the four ADAPTER_GROUPS of a layer: q|k|v, o, gate|up, down."""
        c = self.config
        D, I, NQ, NKV = c.hidden_size, c.intermediate_size, c.num_attention_heads * c.head_dim, c.num_key_value_heads * c.head_dim
        return ((D, (NQ, NKV, NKV)), (NQ, (D,)), (D, (I, I)), (I, (D,)))

    def _group_place(self, i, g):
        projs, (_, outs) = ADAPTER_GROUPS[g][1], self._group_dims()[g]
        slots = [j for j, p in enumerate(projs) if p in self.adapter_modules[i]]
        col0 = [sum(outs[:j]) for j in range(len(outs))]
        split = tuple((col0[j], outs[j], slots.index(j) if j in slots else None, f"layers.{i}.{p}.lora_B.weight" if j in slots else None)
                      for j, p in enumerate(projs))
        if not slots:
            return _GroupPlace(0, None, (), split)
        planes = slots[-1] + 1
        view = None if len(slots) == planes else slice(slots[0], planes, slots[1] - slots[0] if len(slots) > 1 else 1)
        return _GroupPlace(planes, view, tuple((col0[j], outs[j]) for j in slots), split)

    def _draw_bits(self, i, g, seed, p, M, W, device, row0):
        """The dropout planes of the present adapters of group g of layer i, drawn now (no prefetched set): the group's planes up to the
        highest present slot are generated, the present ones are handed on as a view."""
        pl = self._place[i][g]
        bits = hip.lora_dropout_bits(seed, p, M, W, pl.planes, device, row0=row0)
        return bits if pl.view is None else bits[pl.view]

    def prefetch_lora_bits(self, M, device, row0=0):
        """Generate the NEXT forward's LoRA dropout bit planes (all layers, all adapter groups) on a side stream.  The planes
        are pure functions of (seed, step, layer, group) -- nothing on the main stream feeds them -- so the caller starts
        this before the item Q-Former's forward, whose small launches leave most of the chip idle.  From the second step on the
        planes are already there: the decoder's backward regenerates them for the following step the moment it has finished with
        this step's (`_prefetch_next_step`), under the Q-Former's backward.  The planes are allocated on the caller's stream (the
        caching allocator keys blocks by stream) and written on the side stream after it has caught up with the caller's stream."""
        p = self._drop_p()
        if p <= 0.0 or not torch.is_grad_enabled():
            self._release_prefetched(device)
            return
        pre = self._bits_pre
        if pre is not None and pre["step"] == self._lora_step and pre["M"] == M and pre["row0"] == int(row0) and pre["p"] == p:
            return                                 # made under the previous step's backward
        self._release_prefetched(device)
        main = torch.cuda.current_stream(device)
        if self._bits_stream is None:
            self._bits_stream = torch.cuda.Stream(device=device)
        planes = {(i, g): torch.empty((self._place[i][g].planes, M, hip.lora_bits_ld(W)), dtype=torch.uint8, device=device)
                  for i in range(self.config.num_hidden_layers) for g, (W, outs) in enumerate(self._group_dims()) if self._place[i][g].planes}
        # token-packed copies for the backward's token reductions (hip.lora_reduce's ring kernel), made on the side stream as well
        packed = {}
        if lora_bits_t_sizes(M) and lora_rank_rule(self.config.lora_r)["bits_t"]:
            packed = {(i, g): torch.empty((self._place[i][g].planes, M // 32, hip.lora_bits_t_ld(W)), dtype=torch.int32, device=device)
                      for i in range(self.config.num_hidden_layers) for g, (W, outs) in enumerate(self._group_dims())
                      if lora_bits_t_sizes(W=W) and self._place[i][g].planes}
        self._bits_stream.wait_stream(main)
        self._generate_bits(planes, packed, self._lora_step, M, device, int(row0), p)

    def _release_prefetched(self, device=None):
        """Drop a prefetched plane set that no forward will consume (last partial batch of an epoch, train -> eval, a different
        micro-batch).  The planes were allocated on the caller's stream but are WRITTEN on the side stream: the caller's stream
        first waits for the generator's last event, so the caching allocator cannot hand the blocks to main-stream tensors while
        the side stream is still writing masks into them."""
        pre, self._bits_pre = self._bits_pre, None
        if pre is not None and pre.get("event_t") is not None:
            torch.cuda.current_stream(device).wait_event(pre["event_t"])

    def _generate_bits(self, planes, packed, step, M, device, row0, p):
        side = self._bits_stream
        with torch.cuda.stream(side):
            # one event per layer: the forward of layer i waits for ITS planes only, so the generator keeps running under the first
            # layers of the decoder when the Q-Former's forward is shorter than it; the token-packed copies (backward only) come last
            events = []
            for i in range(self.config.num_hidden_layers):
                for g, (W, outs) in enumerate(self._group_dims()):
                    if self._place[i][g].planes:
                        hip.lora_dropout_bits(self.lora_dropout_seed(step, i, g), p, M, W, self._place[i][g].planes, device, out=planes[(i, g)], row0=row0)
                events.append(side.record_event())
            for (i, g), bt in packed.items():
                hip.lora_bits_transpose(planes[(i, g)], self._group_dims()[g][0], out=bt)
            ev_t = side.record_event()
        self._bits_pre = {"step": step, "M": M, "planes": planes, "packed": packed, "events": events, "event_t": ev_t, "row0": int(row0), "p": p}

    def _prefetch_next_step(self, cur, device):
        """Called by the decoder's backward when it has consumed this step's planes: the next step's are written into the SAME buffers
        on the side stream (which first waits for the main stream to get here), under the Q-Former's backward and the optimizer."""
        if not switches.bits_next or not self.training:
            return
        if self.sample_offset is not None:
            # micro-batching / explicit shards: the next forward's first row is not this one's, so planes written here would only be
            # thrown away (and every backward would generate a full set for nothing)
            return
        self._bits_stream.wait_stream(torch.cuda.current_stream(device))
        self._generate_bits(cur["planes"], cur["packed"], self._lora_step, cur["M"], device, cur["row0"], cur["p"])

    def _lora_bcomb(self, pack, device, paired_qkv=False, paired_gu=False):
        """Second-K-range operands of the merged projection launches: y[q|k|v] = h W^T + [t_q|t_k|t_v] Bc^T with
        Bc [N, 16 nad] block-diagonal (rows of adapter a carry B_a in columns 16a..16a+15, zeros elsewhere -- exact zeros, so
        the sum is bit-identical to the per-adapter launches).  q|k|v and gate|up each leave as ONE launch that reads its
        input once (1.09 -> 1.01 ms and 1.58 -> 1.49 ms per layer at C4).  The zero blocks are written once; each step
        refreshes the diagonal blocks from the bf16 shadow with one multi-tensor copy.  paired_qkv / paired_gu: the forward runs the
        fused q/k-norm + RoPE / paired SwiGLU epilogue and reads the operand with its rows in that launch's order ("qkvP" / "guP");
        the per-layer views are made of the form the plan reads only."""
        # Placement: the operand has r columns per PRESENT adapter of the group (the adapted layers share one placement, so one
        # [adapted layers, N, r * present] tensor per group serves them); a layer without an adapter in the group has None there.
        c = self.config
        r, I, L = c.lora_r, c.intermediate_size, c.num_hidden_layers
        dims = self._group_dims()
        if self._bcomb is None or self._bcomb["dev"] != torch.device(device) or self._bcomb["pack"] is not pack:
            # slab of layer i inside the group's tensor, or None
            slab = {g: dict((i, k) for k, i in enumerate(i for i in range(L) if self._names[i][g].b)) for g in (0, 2)}
            qkv, gu = (torch.zeros((len(slab[g]), sum(dims[g][1]), max(nads) * r), dtype=BF16, device=device) if slab[g] else None
                       for g, nads in ((0, self._nad_qkv), (2, self._nad_gu)))
            dst, src = [], []
            for i in range(L):
                for comb, g in ((qkv, 0), (gu, 2)):
                    for j, (bname, (col, n)) in enumerate(zip(self._names[i][g].b, self._place[i][g].cols)):
                        dst.append(comb[slab[g][i], col:col + n, j * r:(j + 1) * r]); src.append(pack.w16(bname))
            self._bcomb = {"dev": torch.device(device), "pack": pack, "qkv3": qkv, "gu3": gu, "dst": dst, "src": src, "slab": slab}
        bc = self._bcomb
        if bc["dst"]:
            torch._foreach_copy_(bc["dst"], bc["src"])
        rp = self._qk_row_perm(device) if switches.fuse_qk_rope else None
        qkvP = bc["qkv3"].index_select(1, rp) if (rp is not None and bc["qkv3"] is not None) else None      # rows paired like fz["qkvP"]
        guP = (bc["gu3"].index_select(1, self._swiglu_rows(I, device)) if (switches.fuse_swiglu_gemm and I % 128 == 0 and bc["gu3"] is not None) else None)

        def per_layer(t3, g):
            slab = bc["slab"][g]
            return [t3[slab[i]] if i in slab else None for i in range(L)] if t3 is not None else none
        none = (None,) * L
        bc["qkv"], bc["qkvP"] = (none, per_layer(qkvP, 0)) if paired_qkv else (per_layer(bc["qkv3"], 0), none)
        bc["gu"], bc["guP"] = (none, per_layer(guP, 2)) if paired_gu else (per_layer(bc["gu3"], 2), none)
        return bc["qkv"], bc["gu"]

    def _lora_transposes(self, pack):
        """A^T (per adapter group) and B^T (per adapter) of every layer for the backward, refreshed by ONE launch per
        backward (308 separate 5 us launches before).  The table is built once per pack: the sources are views of the pack's
        persistent bf16 shadow."""
        bt = getattr(self, "_lt", None)
        if bt is None or bt[0] is not pack:
            names, srcs = [], []
            for groups in self._names:
                for g in groups:
                    if not g.a:            # no adapter in this group of this layer
                        continue
                    names.append(g.a)
                    srcs.append(pack.fused16(list(g.a)) if len(g.a) > 1 else pack.w16(g.a[0]))
                    for bname in g.b:
                        names.append(bname)
                        srcs.append(pack.w16(bname))
            bt = (pack, names, hip.BatchedTranspose(srcs))
            self._lt = bt
        outs = bt[2].run()
        return dict(zip(bt[1], outs))

    def _norm_lora_down(self, x, w, eps, i, g, pack, sc, seed, p, pre=None, row0=0):
        """(h, rstd, t, bits) = RMSNorm forward + _lora_down of the present adapters of group g of layer i, which read h, as one kernel
        (ur_rmsnorm_lora_fwd)."""
        bits = pre
        if bits is None and p > 0.0:
            bits = self._draw_bits(i, g, seed, p, x.shape[0], x.shape[1], x.device, row0)
        h, rstd, t = hip.rmsnorm_lora_fwd(x, w, eps, [pack.w16(n) for n in self._names[i][g].a], alpha=sc / (1.0 - p), bits=bits)
        return h, rstd, t, bits

    def _lora_down(self, xin, i, g, pack, sc, seed, p, pre=None, row0=0):
        """(t, bits): t[M, nb*r] = s * dropout_j(x) A_j^T for the nb present adapters of group g of layer i, which share the input x (one
        dropped-flag bit plane per adapter -- the plane at the module's slot of the group's generator stream -- made once here and kept
        for the backward)."""
        bits = pre
        if bits is None and p > 0.0:
            bits = self._draw_bits(i, g, seed, p, xin.shape[0], xin.shape[1], xin.device, row0)
        t = hip.lora_project(xin, [pack.w16(n) for n in self._names[i][g].a], alpha=sc / (1.0 - p), bits=bits)
        return t, bits

    def _lora_scale(self):
        """s of y = W x + s B A x: lora_alpha / r, or peft's rank-stabilised lora_alpha / sqrt(r) (use_rslora)"""
        c = self.config
        if not self.use_lora:
            return 0.0
        return c.lora_alpha / math.sqrt(c.lora_r) if getattr(c, "use_rslora", False) else c.lora_alpha / c.lora_r

    def _plan(self, M, S, dev, pack, fz):
        """Every launch choice that is the same for all layers of a forward over M = B * S tokens (see _Plan)."""
        c, sw = self.config, switches
        D, I, hd, r = c.hidden_size, c.intermediate_size, c.head_dim, c.lora_r
        NQ, NKV = c.num_attention_heads * hd, c.num_key_value_heads * hd
        lora = pack is not None
        # the second K ranges of the merged launches: r columns per PRESENT adapter of the group, one value per kind of layer (a layer
        # outside layers_to_transform, or a group nobody targets, has none: K2 = 0, R2 = S2 = None)
        nad_qkv, nad_gu = (self._nad_qkv, self._nad_gu) if lora else ([0], [0])
        rule = lora_rank_rule(r, sw, max(nad_qkv[-1], nad_gu[-1])) if lora else lora_rank_rule(r, sw)
        merged = not lora or rule["merged"]
        # q/k-norm + RoPE inside the q|k|v launch (the raw q, k are never written or re-read) when the persistent GEMM takes it
        fuse_rope = (sw.fuse_qk_rope and hd == 128 and fz["qk_norm_fusable"] and merged and
                     all(hip.gemm_qkrope_supported(M, NQ + 2 * NKV, D, n * r, S, NQ, NKV, dev) for n in nad_qkv))
        swiglu = "alone"
        if lora and not merged and sw.swiglu_fwd_fused:
            swiglu = "up"
        elif lora and merged and sw.fuse_swiglu_gemm and I % 128 == 0 and all(hip.gemm_swiglu_paired_supported(M, I, D, n * r, dev) for n in nad_gu):
            swiglu = "pair"
        elif lora and rule["swiglu_lora"] and I % 128 == 0:
            swiglu = "lora"
        # the attention output's rows are padded by 64 columns when their length is a power of two: the kernels that stream it
        # in 128-byte column chunks (the o_proj adapter's projection and its token reduction) otherwise keep every request in
        # flight on the same bytes of a 4 KiB-strided row, i.e. on a few memory channels (lora_project_ring_kernel: 141 -> 104 us)
        pad_att = sw.pad_att and (NQ & (NQ - 1)) == 0 and NQ >= 1024
        # switches.rope_bwd_fused unset: from the roped outputs only
        in_dq = hd == 128 and (sw.rope_bwd_fused is not False if fuse_rope else sw.rope_bwd_fused is True)
        mlp_recompute = None if not merged else ("pair" if swiglu == "pair" else ("merged" if lora else "plain"))
        return _Plan(merged=merged, fuse_norm=rule["fuse_norm"] and lora and D == 1024, fuse_rope=fuse_rope, swiglu=swiglu,
                     pad_att=pad_att, bits_one_event=sw.bits_one_event, mlp_recompute=mlp_recompute, rope_bwd_in_dq=in_dq,
                     rope_k_in_dkv=sw.rope_k_fused, bits_t=(rule["bits_t"] if lora else sw.bits_t) and lora_bits_t_sizes(M))

    def _forward_impl(self, item_tokens16, input_ids, mask_u8, first_special_id, keep=True):
        c = self.config
        dev = input_ids.device
        fz, pack = self._operands(dev)
        B, S = input_ids.shape
        D, I, nq, nkv, hd, r = c.hidden_size, c.intermediate_size, c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.lora_r
        NQ, NKV = nq * hd, nkv * hd
        M = B * S
        plan = self._plan(M, S, dev, pack, fz)
        # LoRA operands: without adapters every projection below is the same call with R2 = S2 = None
        none = (None,) * len(fz["layers"])
        bc_qkv = bc_gu = bc_qkvP = bc_guP = none      # per layer: block-diagonal B of the merged launches (P: rows paired like fz's qkvP / guP)
        w16 = pack.w16 if pack is not None else (lambda name: None)
        if pack is not None:
            pack.refresh_shadow()
            if plan.merged:
                bc_qkv, bc_gu = self._lora_bcomb(pack, dev, paired_qkv=plan.fuse_rope, paired_gu=plan.swiglu == "pair")
                bc_qkvP, bc_guP = self._bcomb["qkvP"], self._bcomb["guP"]
        eps, sc = c.rms_norm_eps, self._lora_scale()
        cos, sin = self._rope_tables(S, dev)
        T = item_tokens16.shape[1]
        tok = item_tokens16.detach().contiguous() if T > 0 else None
        x = hip.embed_inject_fwd(fz["embed"], input_ids, tok, first_special_id).view(M, D)
        pdrop = self._drop_p()
        step = self._lora_step
        if pdrop > 0.0:
            self._lora_step += 1
        saved = {"B": B, "S": S, "T": T, "ids": input_ids, "first": first_special_id, "mask": mask_u8, "layers": [],
                 "pdrop": pdrop, "step": step, "plan": plan, "fz": fz, "pack": pack}
        row0 = self.first_sample(B) * S                # token rows that precede this shard in the global minibatch
        pre, self._bits_pre = self._bits_pre, None
        if pre is not None and not (pdrop > 0.0 and pre["step"] == step and pre["M"] == M and pre["row0"] == row0 and pack is not None):
            self._bits_pre = pre
            self._release_prefetched(dev)           # not this forward's planes: order their last writes before the blocks are reused
            pre = None
        pre_events = None
        if pre is not None:
            saved["bits_t"] = pre.get("packed", {})                      # (layer, group) -> token-packed copy for the backward
            saved["bits_t_event"] = pre["event_t"]
            saved["bits_pre"] = pre                                      # (its buffers take the next step's planes after the backward)
            pre_events = pre["events"]                                   # planes prefetched on the side stream, one event per layer
            pre = pre["planes"]
        place = self._place

        def bp(i, g):
            """the prefetched planes of the present adapters of group g of layer i (a view of the group's planes), or None"""
            if pre is None:
                return None
            v = place[i][g].view
            return pre[(i, g)] if v is None else pre[(i, g)][v]

        def lora_down(xin, i, g):
            """(t, bits) of adapter group g of layer i on its input xin; (None, None) without adapters"""
            if pack is None or not place[i][g].planes:
                return None, None
            return self._lora_down(xin, i, g, pack, sc, self.lora_dropout_seed(step, i, g), pdrop, bp(i, g), row0=row0)

        def norm_lora_down(xin, w, i, g):
            """(h, rstd, t, bits): RMSNorm and lora_down of its output, as one kernel when the plan says so"""
            if plan.fuse_norm and place[i][g].planes:      # (h is written once, never re-read by a projection kernel)
                return self._norm_lora_down(xin, w, eps, i, g, pack, sc, self.lora_dropout_seed(step, i, g), pdrop, bp(i, g), row0=row0)
            h, rstd = hip.rmsnorm_fwd(xin, w, eps)
            return (h, rstd) + lora_down(h, i, g)      # t [M, nad * r] = s * dropout(h) A^T

        for i, fl in enumerate(fz["layers"]):
            nm = self._names[i]
            L = {"x": x}
            if pre_events is not None:
                torch.cuda.current_stream(dev).wait_event(pre_events[-1] if (i == 0 and plan.bits_one_event) else pre_events[i])
            qkv = None if plan.fuse_rope else torch.empty((M, NQ + 2 * NKV), dtype=BF16, device=dev)
            h, rstd1, t_qkv, L["bits_qkv"] = norm_lora_down(x, fl["ln1"], i, 0)
            if plan.fuse_rope:
                q_r, k_r, v2, rstd_qk = hip.gemm_qkv_rope(h, fl["qkvP"], fl["qn"], fl["kn"], cos, sin, S, NQ, NKV, eps, R2=t_qkv, S2=bc_qkvP[i])
                v4 = v2.view(B, S, nkv, hd)
                L.update(q_r=q_r, k_r=k_r, rstd_qk=rstd_qk)
            else:
                if plan.merged or t_qkv is None:
                    hip.gemm(h, fl["qkv"], out=qkv, R2=t_qkv, S2=bc_qkv[i])        # one launch, block-diagonal B (none: no adapter here)
                else:
                    for col, n, j, bname in place[i][0].split:      # one launch per projection; j: its adapter among the present ones
                        hip.gemm(h, fl["qkv"][col:col + n], out=qkv[:, col:col + n], R2=None if j is None else t_qkv[:, j * r:(j + 1) * r],
                                 S2=None if j is None else w16(bname))
                q_r, k_r = hip.qknorm_rope_fwd(qkv, fl["qn"], fl["kn"], cos, sin, S, nq, nkv, hd, eps)
                v4 = qkv[:, NQ + NKV:].view(B, S, nkv, hd)
            att_out = torch.empty((M, NQ + 64), dtype=BF16, device=dev)[:, :NQ].view(B, S, nq, hd) if plan.pad_att else None
            att, actx = hip.attn_fwd(q_r.view(B, S, nq, hd), k_r.view(B, S, nkv, hd), v4, causal=True, key_mask=mask_u8, out=att_out)
            att2 = att.view(M, NQ)
            t_o, L["bits_o"] = lora_down(att2, i, 1)
            x2 = hip.gemm(att2, fl["o"], residual=x, R2=t_o, S2=w16(nm[1].b[0]) if t_o is not None else None)
            gu = torch.empty((M, 2 * I), dtype=BF16, device=dev)
            h2, rstd2, t_gu, L["bits_gu"] = norm_lora_down(x2, fl["ln2"], i, 2)
            # (a layer without a gate / up adapter under per-projection launches runs the group as the adapter-free model does: one launch,
            # SwiGLU on its own; likewise the fused SwiGLU + down projection needs a down adapter in THIS layer)
            swiglu = plan.swiglu
            if (swiglu == "up" and t_gu is None) or (swiglu == "lora" and not nm[3].a):
                swiglu = "alone"
            act = torch.empty((M, I), dtype=BF16, device=dev) if swiglu in ("pair", "up") else None
            if swiglu == "pair":            # ONE launch: gate|up (standard order, for the backward) and act = silu(gate) * up from its registers
                hip.gemm(h2, fl["guP"], out=gu, R2=t_gu, S2=bc_guP[i], swiglu_paired=act)
            elif plan.merged or t_gu is None:
                hip.gemm(h2, fl["gu"], out=gu, R2=t_gu, S2=bc_gu[i])            # one launch, block-diagonal B (none: no adapter here)
            else:
                # gate first; under "up" the up projection's epilogue then reads the gate tile and writes act = silu(gate) * up beside up
                for col, n, j, bname in place[i][2].split:
                    hip.gemm(h2, fl["gu"][col:col + n], out=gu[:, col:col + n], R2=None if j is None else t_gu[:, j * r:(j + 1) * r],
                             S2=None if j is None else w16(bname), swiglu_fwd=(gu[:, :I], act) if (col == I and swiglu == "up") else None)
            if swiglu == "lora":      # act and t_d = s * dropout(act) A_d^T from one pass over gate|up (ur_swiglu_lora_fwd)
                bits_d = bp(i, 3)
                if bits_d is None and pdrop > 0.0:
                    bits_d = hip.lora_dropout_bits(self.lora_dropout_seed(step, i, 3), pdrop, M, I, 1, dev, row0=row0)
                act, t_d = hip.swiglu_lora_fwd(gu, I, w16(nm[3].a[0]), alpha=sc / (1.0 - pdrop), bits=bits_d)
                L["bits_d"] = bits_d
            else:
                if swiglu == "alone":
                    act = hip.swiglu_fwd(gu, I)
                t_d, L["bits_d"] = lora_down(act, i, 3)
            x3 = hip.gemm(act, fl["d"], residual=x2, R2=t_d, S2=w16(nm[3].b[0]) if t_d is not None else None)
            L.update(rstd1=rstd1, qkv=qkv, actx=actx, att=att2, x2=x2, rstd2=rstd2, gu=gu, act=act,      # (qkv is None under the fused q/k-norm + RoPE epilogue)
                     t_qkv=t_qkv, t_o=t_o, t_gu=t_gu, t_d=t_d)
            # (recompute_mlp = True: every layer; an int k: layers 0 .. k - 1 only -- as much memory as the shape needs, no more recomputation than that)
            if self.recompute_mlp and keep and (self.recompute_mlp is True or i < int(self.recompute_mlp)):
                # memory for time: gate|up and act (2 x [M, 3I] bf16 over the stack: 67 GB at C4) are dropped and rebuilt in the
                # backward by the very launch that made them (bit-identical: same kernel, same operands).
                if plan.mlp_recompute is not None:
                    L.update(gu=None, act=None, mlp_recompute=plan.mlp_recompute, bc_gu=bc_guP[i] if plan.mlp_recompute == "pair" else bc_gu[i])
            if self.keep_norm_outputs:       # 2 x [M,D] bf16 per layer (15 GB at C4) instead of two RMSNorm recomputes
                L.update(h=h, h2=h2)
            if keep:
                saved["layers"].append(L)
            x = x3
        if self.pooling != "mean":      # final RMSNorm + mask-aware pooling in one pass; the backward recomputes rstd from the row
            pooled = hip.pool_norm_fwd(x.view(B, S, D), fz["norm"], eps, mask_u8, self.pooling)
            if not keep:
                return pooled, None
            saved["xf"], saved["pooling"] = x, self.pooling
            return pooled, saved
        last, rstd_f = hip.rmsnorm_fwd(x, fz["norm"], eps)
        pooled, _ = hip.mean_pool_fwd(last.view(B, S, D))
        if not keep:
            return pooled, None
        saved["xf"], saved["rstd_f"] = x, rstd_f
        return pooled, saved

    def _backward_impl(self, saved, d_pooled):
        c = self.config
        fz, pack = saved["fz"], saved["pack"]      # what the forward ran on (merged or adapter-free operands: pack is None)
        plan = saved["plan"]
        B, S, T = saved["B"], saved["S"], saved["T"]
        D, I, nq, nkv, hd, r = c.hidden_size, c.intermediate_size, c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.lora_r
        NQ, NKV = nq * hd, nkv * hd
        M = B * S
        eps, sc = c.rms_norm_eps, self._lora_scale()
        dev = d_pooled.device
        cos, sin = self._rope_tables(S, dev)
        if saved.get("pooling") is not None:      # (the rule the forward ran under, and its mask)
            dx = hip.pool_norm_bwd(d_pooled.contiguous().to(F32), saved["xf"].view(B, S, D), fz["norm"], eps, saved["mask"],
                                   saved["pooling"]).view(M, D)
        else:
            dlast = hip.mean_pool_bwd(d_pooled.contiguous().to(F32), S).view(M, D)
            dx = hip.rmsnorm_bwd(dlast, saved["xf"], fz["norm"], saved["rstd_f"])
        touched = []

        pdrop, step = saved["pdrop"], saved["step"]
        lt = self._lora_transposes(pack) if pack is not None else None      # name(s) -> transposed bf16 operand

        packed_bits = saved.get("bits_t", {})
        if saved.get("bits_t_event") is not None:
            torch.cuda.current_stream(dev).wait_event(saved["bits_t_event"])
        place = self._place      # per layer and adapter group: (first output column, width) of every present adapter, plane views

        def lora_grads(dy, t, xin, i, g, bits):
            """Adapter group g of layer i: dB_p = dy_p^T t_p ; tb = s * dy B ; dA_p = tb_p^T dropout_p(x).  Returns tb [M, nad * r] (bf16)."""
            a_names, bnames, cols = self._names[i][g].a, self._names[i][g].b, place[i][g].cols
            nb = len(bnames)
            touched.extend(bnames + a_names)
            gA = pack.fusedg(a_names) if nb > 1 else pack.g32(a_names[0])
            gB = pack.fusedg(bnames) if nb > 1 else pack.g32(bnames[0])            # [sum n, r]: adapter ranges in order
            tb = hip.lora_bgrad(dy, t, [lt[b] for b in bnames], cols, gB, alpha=sc)     # dB and tb, dy read once
            bits_t = packed_bits.get((i, g)) if bits is not None else None             # the prefetched token-packed flags
            if bits_t is not None and place[i][g].view is not None:
                bits_t = bits_t[place[i][g].view]                                      # (the present adapters' planes of the group's)
            if bits is not None and bits_t is None and plan.bits_t and lora_bits_t_sizes(W=xin.shape[1]):
                bits_t = hip.lora_bits_transpose(bits, xin.shape[1])          # (no prefetch this step: made here)
            hip.lora_reduce(xin, tb, gA, nad=nb, alpha=1.0 / (1.0 - pdrop), bits=bits, bits_t=bits_t)
            return tb

        def proj_bwd(dy, wT, xin, i, g, L, swiglu=None):
            """Backward of the projections of adapter group g of layer i (input xin, output gradient dy): the adapters' gradients
            (lora_grads), then dx = dy W + sum_j mask_j * (tb_j A_j): the adapters' part joins the main reduction when there is no
            dropout, and is a masked rank-r epilogue (ur_gemm drop_bits) when there is.  Without adapters: dx = dy W.
            swiglu = (gu, dgu): dx is d(act) and leaves the GEMM as dgate | dup (SwiGLU backward in the epilogue: d(act) is never stored)."""
            tb = AT = drop = None
            if pack is not None and place[i][g].planes:
                key, a_names = ADAPTER_GROUPS[g][0], self._names[i][g].a
                bits = L["bits_" + key]
                tb = lora_grads(dy, L["t_" + key], xin, i, g, bits)
                AT = lt[a_names]
                drop = (bits, pdrop, r) if bits is not None else None
            return hip.gemm(dy, wT, R2=tb, S2=AT, drop=drop, swiglu_bwd=swiglu)

        scratch = {}
        for i in reversed(range(len(fz["layers"]))):
            fl, L = fz["layers"][i], saved["layers"][i]
            x, x2, gu, qkv = L["x"], L["x2"], L["gu"], L["qkv"]
            # ---- MLP: x3 = x2 + down(silu(gate) * up)
            act = L["act"]
            h2 = L["h2"] if "h2" in L else hip.rmsnorm_fwd(x2, fl["ln2"], eps)[0]          # kept, or recomputed
            if L.get("mlp_recompute"):           # recompute_mlp: one [M, 2I] + [M, I] scratch pair serves every layer
                if "gu" not in scratch:
                    scratch["gu"] = torch.empty((M, 2 * I), dtype=BF16, device=dev)
                    scratch["act"] = torch.empty((M, I), dtype=BF16, device=dev)
                gu, act = scratch["gu"], scratch["act"]
                if L["mlp_recompute"] == "pair":
                    hip.gemm(h2, fl["guP"], out=gu, R2=L["t_gu"], S2=L["bc_gu"], swiglu_paired=act)
                else:            # "merged" / "plain" (no adapters)
                    hip.gemm(h2, fl["gu"], out=gu, R2=L["t_gu"], S2=L["bc_gu"])
                    hip.swiglu_fwd(gu, I, out=act)
            dgu = torch.empty_like(gu)
            proj_bwd(dx, fl["dT"], act, i, 3, L, swiglu=(gu, dgu))
            dh2 = proj_bwd(dgu, fl["guT"], h2, i, 2, L)
            dx2 = hip.rmsnorm_bwd(dh2, x2, fl["ln2"], L["rstd2"], add=dx)
            # ---- attention: x2 = x + o(attn)
            datt = proj_bwd(dx2, fl["oT"], L["att"], i, 1, L)
            dqkv = torch.empty((M, NQ + 2 * NKV), dtype=BF16, device=dev)
            dk_r = torch.empty((M, NKV), dtype=BF16, device=dev)
            datt4, dk4, dv4 = datt.view(B, S, nq, hd), dk_r.view(B, S, nkv, hd), dqkv[:, NQ + NKV:].view(B, S, nkv, hd)
            if not plan.rope_bwd_in_dq:      # the q/k-norm + RoPE backward as its own pass over dq | dk
                dq_r = torch.empty((M, NQ), dtype=BF16, device=dev)
                hip.attn_bwd(L["actx"], datt4, dq=dq_r.view(B, S, nq, hd), dk=dk4, dv=dv4)
                if plan.fuse_rope:
                    hip.qknorm_rope_bwd_roped(dq_r, dk_r, L["q_r"], L["k_r"], L["rstd_qk"], fl["qn"], fl["kn"], cos, sin, dqkv, S, nq, nkv, hd)
                else:
                    hip.qknorm_rope_bwd(dq_r, dk_r, qkv, fl["qn"], fl["kn"], cos, sin, dqkv, S, nq, nkv, hd, eps)
            elif plan.fuse_rope:
                # the forward ran q/k-norm + RoPE in the q|k|v launch: no raw q, k exist; the rows are recovered from the roped outputs.
                # The q heads' backward rides in the dQ kernel's store (its lanes own whole rows of q_r, which it has just read as
                # its q operand): dq never makes the round trip through HBM.
                # (the k heads' likewise in the dK/dV kernel's store; dk_r is scratch for the shapes the generated kernels do not take)
                hip.attn_bwd(L["actx"], datt4, dk=dk4, dv=dv4, rope_q=(L["q_r"], fl["qn"], cos, sin, eps, dqkv[:, :NQ]), rope_rstd=(L["rstd_qk"], 0),
                             rope_k=(L["k_r"], fl["kn"], nq, dqkv[:, NQ:NQ + NKV]) if plan.rope_k_in_dkv else None)
                if not plan.rope_k_in_dkv:
                    hip.qknorm_rope_bwd_roped_k(dk_r, L["k_r"], L["rstd_qk"], nq, fl["kn"], cos, sin, dqkv[:, NQ:NQ + NKV], S, nkv, hd)
            else:
                # from the RAW projection (switches.rope_bwd_fused = True): the dQ kernel carries the q-norm + RoPE backward of the q
                # heads (its lanes own whole rows) and writes straight into dqkv; the stand-alone kernel is left with the k heads
                # (nq = 0, operands offset to the k columns)
                hip.attn_bwd(L["actx"], datt4, dk=dk4, dv=dv4, rope_q=(qkv[:, :NQ], fl["qn"], cos, sin, eps, dqkv[:, :NQ]))
                hip.qknorm_rope_bwd(dk_r, dk_r, qkv[:, NQ:], fl["qn"], fl["kn"], cos, sin, dqkv[:, NQ:], S, 0, nkv, hd, eps)
            h = L["h"] if "h" in L else hip.rmsnorm_fwd(x, fl["ln1"], eps)[0]              # kept, or recomputed
            dh = proj_bwd(dqkv, fl["qkvT"], h, i, 0, L)
            dx = hip.rmsnorm_bwd(dh, x, fl["ln1"], L["rstd1"], add=dx2)
            L.clear()
            if self.grad_ready_hook is not None:      # dp.GradBuckets: layer i's LoRA gradients are final
                self.grad_ready_hook(i)
        if pack is not None:
            pack.publish_grads(touched)
        if saved.get("bits_pre") is not None and self._bits_pre is None:
            self._prefetch_next_step(saved.pop("bits_pre"), dev)
        if T > 0:
            return hip.inject_bwd(dx.view(B, S, D), saved["ids"], saved["first"], T)
        return None
