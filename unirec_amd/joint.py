"""Drop-in for the model/loss part of ``training/train_item_individual_token_joint.py``:
``MultiModalQwenEmbedding`` (:88-212), ``InfoNCELoss`` (:326-352), MRR (:392-419) and
``MultiModalTrainer.compute_loss`` (:482-498), all on the HIP path; ``JointTrainer`` is the optimisation step HF Trainer runs
around that loss with the reference's ``TrainingArguments`` (:755-773): gradient-norm clipping, AdamW, the warm-up schedule.

Differences that are deliberate and documented:
  * no network here: the Qwen3 backbone is built from a ``Qwen3Config`` (random init or weights the
    caller loads with load_state_dict) instead of ``AutoModel.from_pretrained``; ``.tokenizer`` is a
    minimal table of the history special tokens unless a real tokenizer is handed in.
  * ``num_history_items`` / ``num_query_tokens_per_item`` are constructor arguments (the reference
    hard-codes 10 and 2, :93-94, which cannot express BASELINE's hist=50/100).
  * the python triple loop with one host sync per (item, query, sample) (:160-171) is one kernel.
"""
import json
import math
import os
import re

import torch
import torch.nn as nn

from . import hip
from .qwen3 import Qwen3Config, Qwen3LoRAModel, normalize_lora_layers, normalize_lora_targets, normalize_pooling

BF16, F32 = torch.bfloat16, torch.float32


class HistoryTokenTable:
    """Stand-in for the tokenizer methods the joint model touches (:106-116,163)."""

    def __init__(self, base_vocab, num_history_items, num_query_tokens_per_item):
        self.base_vocab = base_vocab
        self.history_tokens = [f"<|history_item_{i}_query_{j}|>" for i in range(num_history_items)
                               for j in range(num_query_tokens_per_item)]
        self._ids = {t: base_vocab + k for k, t in enumerate(self.history_tokens)}
        self.pad_token = "<|endoftext|>"

    def __len__(self):
        return self.base_vocab + len(self.history_tokens)

    def convert_tokens_to_ids(self, name):
        return self._ids[name]

    def save_pretrained(self, save_directory):
        with open(os.path.join(save_directory, "history_tokens.json"), "w") as f:
            json.dump(self._ids, f)


# peft.LoraConfig fields this package does not implement: accepted only with the value under which they do nothing
_LORA_INERT = (("rank_pattern", lambda v: not v, "empty (one rank for all modules)"),
               ("alpha_pattern", lambda v: not v, "empty (one lora_alpha for all modules)"),
               ("bias", lambda v: v == "none", '"none" (no bias is trained)'),
               ("use_dora", lambda v: not v, "False"),
               ("fan_in_fan_out", lambda v: not v, "False"),
               ("modules_to_save", lambda v: v is None or len(v) == 0, "None or empty"),
               ("layers_pattern", lambda v: v is None or len(v) == 0, "None or empty"),
               ("exclude_modules", lambda v: v is None or len(v) == 0, "None or empty"))
_ABSENT = object()


def apply_lora_config(cfg, lora_config):
    """Copy a ``peft.LoraConfig``-like object or dict into a Qwen3Config: r, lora_alpha, lora_dropout, target_modules,
    layers_to_transform and use_rslora are honoured (the placement is validated here, against this config's layer count); the fields
    of _LORA_INERT raise a ValueError that names the field unless they hold their inert value.  An absent field is never an error.
    One deviation from peft: an absent / None ``target_modules`` keeps all seven projections (peft would pick q_proj and v_proj for
    the Qwen family) -- the reference's own config names all seven, and that has been this package's behaviour all along."""
    get = (lambda k: lora_config.get(k, _ABSENT)) if isinstance(lora_config, dict) else (lambda k: getattr(lora_config, k, _ABSENT))
    for name, inert, what in _LORA_INERT:
        v = get(name)
        if v is not _ABSENT and not inert(v):
            raise ValueError(f"lora_config.{name} = {v!r} is not supported: only {what} is accepted")
    for src, dst in (("r", "lora_r"), ("lora_alpha", "lora_alpha"), ("lora_dropout", "lora_dropout")):
        if get(src) is not _ABSENT:
            setattr(cfg, dst, get(src))
    targets, layers, rs = get("target_modules"), get("layers_to_transform"), get("use_rslora")
    if targets is not _ABSENT and targets is not None:
        cfg.lora_target_modules = list(normalize_lora_targets(targets))
    if layers is not _ABSENT and layers is not None:
        cfg.lora_layers_to_transform = list(normalize_lora_layers(layers, cfg.num_hidden_layers))
    if rs is not _ABSENT:
        cfg.use_rslora = bool(rs)
    return cfg


def _copy_config(cfg):
    new = Qwen3Config()
    new.__dict__.update(cfg.__dict__)
    return new


def adapter_config_dict(cfg, base_model_name_or_path=None):
    """``adapter_config.json`` in peft's format for the adapters a Qwen3Config describes (what ``PeftModel.save_pretrained`` writes
    next to ``adapter_model.bin``; ``peft.LoraConfig.from_pretrained`` reads it back)."""
    layers = cfg.lora_layers_to_transform
    return {"peft_type": "LORA", "task_type": "FEATURE_EXTRACTION", "base_model_name_or_path": base_model_name_or_path,
            "r": int(cfg.lora_r), "lora_alpha": cfg.lora_alpha, "lora_dropout": float(cfg.lora_dropout),
            "target_modules": list(normalize_lora_targets(cfg.lora_target_modules)),
            "layers_to_transform": None if layers is None else list(normalize_lora_layers(layers, cfg.num_hidden_layers)),
            "use_rslora": bool(cfg.use_rslora), "bias": "none", "inference_mode": True}


def hf_qwen3_config_dict(cfg, dtype=torch.float32):
    """``config.json`` of a ``transformers`` Qwen3Model for the decoder a Qwen3Config describes (no adapter fields: they are folded into
    the weights of a merged export).  rope_theta is given in both spellings: ``rope_parameters`` (transformers 5) and the flat key."""
    return {"architectures": ["Qwen3Model"], "model_type": "qwen3",
            "vocab_size": int(cfg.vocab_size), "hidden_size": int(cfg.hidden_size), "intermediate_size": int(cfg.intermediate_size),
            "num_hidden_layers": int(cfg.num_hidden_layers), "num_attention_heads": int(cfg.num_attention_heads),
            "num_key_value_heads": int(cfg.num_key_value_heads), "head_dim": int(cfg.head_dim), "hidden_act": "silu",
            "rms_norm_eps": float(cfg.rms_norm_eps), "rope_theta": float(cfg.rope_theta),
            "rope_parameters": {"rope_type": "default", "rope_theta": float(cfg.rope_theta)},
            "max_position_embeddings": int(getattr(cfg, "max_position_embeddings", 32768)),
            "attention_bias": False, "attention_dropout": 0.0, "tie_word_embeddings": True, "use_sliding_window": False,
            "initializer_range": float(cfg.initializer_range), "use_cache": True, "dtype": str(dtype).replace("torch.", "")}


_HF_TO_CFG = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "num_key_value_heads",
              "head_dim", "rms_norm_eps", "initializer_range")


def write_hf_checkpoint(save_directory, cfg, state_dict, dtype=torch.float32):
    """``model.safetensors`` (HF key names, tensors as given) and ``config.json``: what
    ``transformers.Qwen3Model.from_pretrained(save_directory, local_files_only=True)`` loads."""
    from safetensors.torch import save_file
    lora = [k for k in state_dict if ".lora_" in k]
    if lora:
        raise ValueError(f"write_hf_checkpoint: {lora[0]} is an adapter tensor; a merged export holds the HF Qwen3Model keys only")
    save_file({k: v.detach().to("cpu", dtype).contiguous() for k, v in state_dict.items()}, os.path.join(save_directory, "model.safetensors"),
              metadata={"format": "pt"})
    with open(os.path.join(save_directory, "config.json"), "w") as f:
        json.dump(hf_qwen3_config_dict(cfg, dtype), f, indent=2)


class MultiModalQwenEmbedding(nn.Module):
    def __init__(self, base_model_name: str = "Qwen/Qwen3-Embedding-0.6B", qformer_model: nn.Module = None, use_lora: bool = True,
                 lora_config=None, qwen_config: Qwen3Config = None, num_history_items: int = 10,
                 num_query_tokens_per_item: int = 2, tokenizer=None, user_qformer: nn.Module = None, pooling: str = None):
        """pooling: "mean" (over all S positions, padding included: the reference's rule), "masked_mean" or "last" (mask-aware: the
        embedding does not depend on the padded length); None keeps qwen_config.pooling.  Anything else raises a ValueError."""
        super().__init__()
        if pooling is not None:
            normalize_pooling(pooling)      # (refused here: before any module is built)
        # U4 (README.md:44-47 / figure (c), no reference code): the User Q-Former's query
        # tokens are injected at <|user_query_k|> specials that follow the history specials.
        self.user_qformer = user_qformer
        self.num_user_query_tokens = 0 if user_qformer is None else int(user_qformer.num_query_tokens)
        self.use_lora = use_lora
        self.num_history_items = num_history_items
        self.num_query_tokens_per_item = num_query_tokens_per_item
        self.qformer_model = qformer_model
        cfg = qwen_config or Qwen3Config()
        if lora_config is not None:      # peft.LoraConfig-like object or dict: every field is honoured or refused by name
            apply_lora_config(cfg, lora_config)
        if pooling is not None:
            cfg.pooling = pooling
        self.base_model_name = base_model_name
        self.base_model = Qwen3LoRAModel(cfg, use_lora=use_lora)
        self.hidden_size = cfg.hidden_size
        if qformer_model is not None and qformer_model.config.hidden_size != self.hidden_size:
            raise ValueError("No projector: Q-Former hidden size must equal the LLM hidden size (:109)")
        base_vocab = cfg.vocab_size
        self.history_tokens = [f"<|history_item_{i}_query_{j}|>" for i in range(num_history_items)
                               for j in range(num_query_tokens_per_item)]
        self.user_tokens = [f"<|user_query_{k}|>" for k in range(self.num_user_query_tokens)]
        if tokenizer is None:
            tokenizer = HistoryTokenTable(base_vocab, num_history_items, num_query_tokens_per_item)
        elif hasattr(tokenizer, "add_special_tokens"):
            # a real tokenizer: extend it exactly as the reference does (:106-118); ids of the added tokens are consecutive
            if getattr(tokenizer, "pad_token", None) is None and getattr(tokenizer, "eos_token", None) is not None:
                tokenizer.pad_token = tokenizer.eos_token
            tokenizer.add_special_tokens({"additional_special_tokens": self.history_tokens + self.user_tokens})
        self.tokenizer = tokenizer
        # ids of the added special tokens are consecutive (tokenizer.add_special_tokens order, :106-119)
        self.first_special_id = int(self.tokenizer.convert_tokens_to_ids(self.history_tokens[0]))
        self.first_user_special_id = self.first_special_id + len(self.history_tokens)
        need = self.first_user_special_id + len(self.user_tokens)
        try:
            need = max(need, len(self.tokenizer))          # :119 resize_token_embeddings(len(tokenizer))
        except TypeError:
            pass
        self.base_model.resize_token_embeddings(max(base_vocab, need))
        if user_qformer is not None and user_qformer.config.hidden_size != self.hidden_size:
            raise ValueError("No projector: User Q-Former hidden size must equal the LLM hidden size")

    def forward(self, input_ids, attention_mask=None, history_field_embeddings=None, history_attention_mask=None,
                user_sequence_tokens=None, user_attention_mask=None):
        self.base_model.refuse_training_while_merged()      # (before the Q-Formers launch anything)
        dev = self.base_model.embed_tokens.weight.device
        input_ids = input_ids.to(dev)
        if attention_mask is not None:
            attention_mask = attention_mask.to(dev)
        item_tokens = None
        if self.use_lora and self.training and input_ids.is_cuda:
            # this step's LoRA dropout bit planes do not depend on any activation: generate them on a side stream under the
            # Q-Former forward(s) below
            self.base_model.prefetch_lora_bits(input_ids.shape[0] * input_ids.shape[1], dev,
                                               row0=self.base_model.first_sample(input_ids.shape[0]) * input_ids.shape[1])
        if history_field_embeddings is not None and history_attention_mask is not None:
            hfe = history_field_embeddings.to(dev)
            ham = history_attention_mask.to(dev)
            bh, num_hist, num_fields, field_dim = hfe.shape
            h16 = self.qformer_model.encode_bf16(hfe.reshape(bh * num_hist, num_fields, field_dim), ham.reshape(bh * num_hist, num_fields))
            if h16.shape[1] != self.num_query_tokens_per_item or num_hist != self.num_history_items:
                raise ValueError("history layout does not match num_history_items x num_query_tokens_per_item")
            item_tokens = h16.reshape(bh, num_hist * self.num_query_tokens_per_item, self.hidden_size)
        if self.user_qformer is not None and user_sequence_tokens is not None:
            u16 = self.user_qformer.encode_bf16(user_sequence_tokens.to(dev), user_attention_mask.to(dev))     # [B,64,D]
            if item_tokens is None:
                item_tokens = torch.zeros((u16.shape[0], len(self.history_tokens), self.hidden_size), dtype=BF16, device=dev)
            item_tokens = torch.cat([item_tokens, u16], dim=1)      # special ids are consecutive: history block, then user block
        return self.base_model.forward_pooled(input_ids, attention_mask, item_tokens, self.first_special_id)

    def load_base_weights(self, state_dict, strict=True):
        """Load a Qwen3 checkpoint (the state_dict of the ``AutoModel`` the reference builds at :98-103) into the frozen
        backbone AFTER the vocabulary was extended: ``embed_tokens.weight`` of the checkpoint has the base vocabulary only,
        its rows are copied and the added special-token rows are kept (load first, resize afterwards in the reference,
        :99-119 -- same result).  Returns (missing, unexpected) like ``load_state_dict``."""
        return self.base_model.load_base_weights(state_dict, strict=strict)

    # ---- peft's calls for a finished run (Qwen3LoRAModel has the arithmetic) ------------------------------------------------------
    def merge_adapter(self):
        self.base_model.merge_adapter()

    def unmerge_adapter(self):
        self.base_model.unmerge_adapter()

    def disable_adapter(self):
        return self.base_model.disable_adapter()

    def merge_and_unload(self):
        self.base_model.merge_and_unload()
        self.use_lora = False
        return self

    def save_pretrained(self, save_directory, merged=False, dtype=torch.float32):
        """merged=False: the adapters (``adapter_model.bin`` + ``adapter_config.json``; without LoRA ``base_model.bin``), the Q-Former, the
        tokenizer files and ``model_config.json`` (which also records the pooling rule).  merged=True: in place of the adapter files a
        decoder ordinary ``transformers`` code loads -- ``model.safetensors`` (HF key names, W + s B A in `dtype`, ``embed_tokens`` with
        its added special-token rows) and
        ``config.json``; the live model is not modified.  from_pretrained() reads either form back."""
        os.makedirs(save_directory, exist_ok=True)
        self.tokenizer.save_pretrained(save_directory)
        if merged:
            write_hf_checkpoint(save_directory, self.base_model.config, self.base_model.merged_state_dict(dtype), dtype)
        elif self.use_lora:
            torch.save(self.base_model.peft_state_dict(), os.path.join(save_directory, "adapter_model.bin"))
            with open(os.path.join(save_directory, "adapter_config.json"), "w") as f:      # peft's own companion of adapter_model.bin
                json.dump(adapter_config_dict(self.base_model.config, self.base_model_name), f, indent=2)
        else:
            torch.save(self.base_model.state_dict(), os.path.join(save_directory, "base_model.bin"))
        torch.save(self.qformer_model.state_dict(), os.path.join(save_directory, "qformer_model.bin"))
        with open(os.path.join(save_directory, "model_config.json"), "w") as f:
            json.dump({"hidden_size": self.hidden_size, "use_lora": self.use_lora, "pooling": self.base_model.pooling}, f, indent=2)
        print(f"Model saved to {save_directory}")

    def load_adapter(self, path_or_state_dict):
        """Adapter tensors written by save_pretrained (a directory, the path of an ``adapter_model.bin``, or its state dict with peft's
        ``base_model.model.`` prefix) into this model's adapters.  A directory's ``adapter_config.json`` must describe this model's
        adapters (rank, scale and placement; the fields this package refuses raise through apply_lora_config); a key that does not fit
        the placement, a wrong shape or a missing tensor raises, naming the key."""
        sd = path_or_state_dict
        if not isinstance(sd, dict):
            path = os.fspath(sd)
            if os.path.isdir(path):
                with open(os.path.join(path, "adapter_config.json")) as f:
                    want, have = adapter_config_dict(apply_lora_config(_copy_config(self.base_model.config), json.load(f))), adapter_config_dict(self.base_model.config)
                for k in ("r", "lora_alpha", "target_modules", "layers_to_transform", "use_rslora"):
                    if want[k] != have[k]:
                        raise ValueError(f"load_adapter: adapter_config.json has {k} = {want[k]!r}, this model was built with {have[k]!r}")
                path = os.path.join(path, "adapter_model.bin")
            sd = torch.load(path, map_location="cpu")
        if not self.base_model.use_lora:
            raise ValueError("load_adapter: this model has no adapters (use_lora=False, or merge_and_unload() removed them)")
        own = dict(self.base_model.lora_named_parameters())
        pre = "base_model.model."
        with torch.no_grad():
            for k, v in sd.items():
                n = k[len(pre):] if k.startswith(pre) else k
                if n not in own:
                    raise KeyError(f"load_adapter: {k} does not fit the adapter placement of this model (no such adapter tensor)")
                if tuple(v.shape) != tuple(own[n].shape):
                    raise ValueError(f"load_adapter: {k} has shape {tuple(v.shape)}, the model's is {tuple(own[n].shape)}")
            missing = [n for n in own if n not in sd and pre + n not in sd]
            if missing:
                raise KeyError(f"load_adapter: {pre + missing[0]} is missing ({len(missing)} adapter tensors are)")
            for k, v in sd.items():
                p = own[k[len(pre):] if k.startswith(pre) else k]
                p.copy_(v.to(p.device, p.dtype))
        if self.base_model.pack is not None:
            self.base_model.pack.mark_dirty()
        return self

    @classmethod
    def from_pretrained(cls, save_directory, qformer_model=None, base_state_dict=None, qwen_config=None, **kwargs):
        """The model save_pretrained wrote to save_directory, in either form.  The adapters' rank, scale and placement come from
        ``adapter_config.json`` (through apply_lora_config: a field this package refuses raises by name), their values from
        ``adapter_model.bin``, the Q-Former's from ``qformer_model.bin``.  The frozen base weights are not part of an adapter directory:
        pass the checkpoint as base_state_dict (or call load_base_weights afterwards) and the decoder's shape as qwen_config.  A merged
        directory holds both (``model.safetensors``, ``config.json``) and gives a model without adapters.  kwargs go to the constructor."""
        with open(os.path.join(save_directory, "model_config.json")) as f:
            model_config = json.load(f)
        use_lora = bool(model_config.get("use_lora", True))
        if kwargs.get("pooling") is None:      # a constructor keyword wins; a directory from before the field pools as it always did
            kwargs["pooling"] = normalize_pooling(model_config.get("pooling", "mean"))
        merged_file = os.path.join(save_directory, "model.safetensors")
        lora_config = None
        if os.path.exists(merged_file):
            use_lora = False
            with open(os.path.join(save_directory, "config.json")) as f:
                hf = json.load(f)
            qwen_config = qwen_config or Qwen3Config()
            for k in _HF_TO_CFG:
                setattr(qwen_config, k, hf[k])
            qwen_config.rope_theta = (hf.get("rope_parameters") or {}).get("rope_theta", hf.get("rope_theta", qwen_config.rope_theta))
            from safetensors.torch import load_file
            base_state_dict = load_file(merged_file)
            tokens_file = os.path.join(save_directory, "history_tokens.json")
            if kwargs.get("tokenizer") is None and os.path.exists(tokens_file):
                # config.json's vocabulary already counts the added special-token rows: the stand-in tokenizer starts where they start
                with open(tokens_file) as f:
                    first = min(json.load(f).values())
                kwargs["tokenizer"] = HistoryTokenTable(first, kwargs.get("num_history_items", 10), kwargs.get("num_query_tokens_per_item", 2))
        elif use_lora:
            with open(os.path.join(save_directory, "adapter_config.json")) as f:
                lora_config = json.load(f)
        elif base_state_dict is None:
            base_state_dict = torch.load(os.path.join(save_directory, "base_model.bin"), map_location="cpu")
        model = cls(qformer_model=qformer_model, use_lora=use_lora, lora_config=lora_config, qwen_config=qwen_config, **kwargs)
        if base_state_dict is not None:
            model.load_base_weights(base_state_dict)
        if use_lora:
            model.load_adapter(os.path.join(save_directory, "adapter_model.bin"))
        if qformer_model is not None:
            qformer_model.load_state_dict(torch.load(os.path.join(save_directory, "qformer_model.bin"), map_location="cpu"))
        return model

    def get_trainable_parameters(self):
        trainable_params = sum(p.numel() for p in self.parameters() if p.requires_grad)
        all_param = sum(p.numel() for p in self.parameters())
        print(f"Trainable params: {trainable_params:,} || All params: {all_param:,} || "
              f"Trainable%: {100 * trainable_params / all_param:.2f}%")
        return trainable_params, all_param


class _InfoNCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, user, pos, neg, neg_mask_u8, temperature):
        scores, inv = hip.cosine_scores(user, pos, neg)
        loss, du = hip.infonce_fwd_bwd(user, pos, neg, neg_mask_u8, scores, inv, temperature, 1.0, need_grad=True)
        ctx.du = du
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        du = ctx.du * g     # scalar upstream gradient (1.0 from loss.backward()); elementwise scale of [B,D]
        return du, None, None, None, None


class _MatryoshkaInfoNCEFn(torch.autograd.Function):
    """The weighted sum of the InfoNCE losses on the nested prefixes ``owner.matryoshka_dims`` of the embeddings: one
    ``hip.mrl_infonce`` (one pass over the candidates for all score planes, one for the whole gradient)."""

    @staticmethod
    def forward(ctx, user, pos, neg, neg_mask_u8, owner):
        loss, plane_loss, du, _, _ = hip.mrl_infonce(user, pos, neg, neg_mask_u8, owner.matryoshka_dims, owner.matryoshka_weights,
                                                     owner.temperature, 1.0, need_grad=True)
        owner.last_plane_loss = plane_loss
        ctx.du = du
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        return ctx.du * g, None, None, None, None


class InfoNCELoss(nn.Module):
    """The reference's InfoNCE loss.  ``matryoshka_dims`` (ascending multiples of 4, the last one the embedding width) makes it the
    Matryoshka form: sum_k matryoshka_weights[k] * InfoNCE(u[:, :d_k], p[:, :d_k], n[..., :d_k]), every prefix renormalised, weights all
    ones unless given (a zero weight keeps the plane's loss in ``last_plane_loss`` and out of the sum and the gradient).
    ``last_plane_loss`` holds the K per-prefix losses of the last call as a device tensor.  None is the plain loss: the same two
    launches and the same bits as ever."""

    def __init__(self, temperature: float = 0.07, matryoshka_dims=None, matryoshka_weights=None):
        super().__init__()
        self.temperature = temperature
        if matryoshka_dims is None:
            if matryoshka_weights is not None:
                raise ValueError("matryoshka_weights needs matryoshka_dims")
            self.matryoshka_dims = self.matryoshka_weights = None
        else:
            self.matryoshka_dims = hip.mrl_dims(matryoshka_dims, "matryoshka_dims")
            self.matryoshka_weights = hip.mrl_weights(matryoshka_weights, len(self.matryoshka_dims), "matryoshka_weights")
            if not float(temperature) > 0:
                raise ValueError(f"temperature must be positive, got {temperature}")
        self.last_plane_loss = None

    def forward(self, user_embeddings, positive_item_embeddings, negative_item_embeddings, negative_masks=None):
        if self.matryoshka_dims is not None and self.matryoshka_dims[-1] != user_embeddings.shape[-1]:
            raise ValueError(f"matryoshka_dims: the last entry must be the embedding width {user_embeddings.shape[-1]}, "
                             f"got {self.matryoshka_dims}")
        u = user_embeddings.contiguous().to(F32)
        dev = u.device
        p = positive_item_embeddings.to(dev, F32).contiguous()
        n = negative_item_embeddings.to(dev, F32).contiguous()
        m = None if negative_masks is None else negative_masks.to(dev).to(torch.uint8).contiguous()
        if self.matryoshka_dims is not None:
            return _MatryoshkaInfoNCEFn.apply(u, p, n, m, self)
        return _InfoNCEFn.apply(u, p, n, m, float(self.temperature))


def mrr_ranks(user_embeddings, positive_item_embeddings, negative_item_embeddings, negative_masks=None, dims=None):
    """(:408-419) cosine scores of [positive; negatives] and the positive's 1-based rank per user.
    dims (ascending multiples of 4, the last one D): scores [K,B,N+1] and ranks [K,B] on the first dims[k] components, from one
    ``hip.mrl_scores`` (the candidates are read once) and ``hip.mrr_rank`` per plane."""
    if dims is not None:
        dims = hip.mrl_dims(dims, "dims", user_embeddings.shape[-1])
    u = user_embeddings.detach().contiguous().to(F32)
    p = positive_item_embeddings.to(u.device, F32).contiguous()
    n = negative_item_embeddings.to(u.device, F32).contiguous()
    m = None if negative_masks is None else negative_masks.to(u.device).to(torch.uint8).contiguous()
    if dims is not None:
        scores, _ = hip.mrl_scores(u, p, n, dims)
        return scores, torch.stack([hip.mrr_rank(scores[k], m) for k in range(len(dims))])
    scores, _ = hip.cosine_scores(u, p, n)
    return scores, hip.mrr_rank(scores, m)


class _CatalogSoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, user, owner, gt, ex):
        ev = owner.evaluator
        loss, row_loss, lse, du, ev._inv = hip.catalog_softmax(user, ev.catalog, gt, owner.temperature, ev._inv, exclude=ex,
                                                                 chunk_rows=owner.chunk_rows, scorer=owner.scorer, grad_scale=1.0,
                                                                 need_grad=True)
        owner.last_lse, owner.last_row_loss = lse, row_loss
        ctx.du = du
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        return ctx.du * g, None, None, None


class _CatalogMrlSoftmaxFn(torch.autograd.Function):
    """The weighted sum of the catalogue softmax losses on the nested prefixes ``owner.matryoshka_dims``: one ``hip.catalog_mrl_softmax``
    over the resident catalogue, read in place; the norm planes are the evaluator's, the ones ``retrieve_funnel`` searches with."""

    @staticmethod
    def forward(ctx, user, owner, gt, ex):
        loss, plane_loss, row_loss, lse, du, _ = hip.catalog_mrl_softmax(user, owner.evaluator.catalog, gt, owner.matryoshka_dims,
                                                                         owner.matryoshka_weights, owner.temperature, owner._norm_planes(),
                                                                         exclude=ex, chunk_rows=owner.chunk_rows, scorer=owner.scorer,
                                                                         grad_scale=1.0, need_grad=True)
        owner.last_lse, owner.last_row_loss, owner.last_plane_loss = lse, row_loss, plane_loss
        ctx.du = du
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        return ctx.du * g, None, None, None


class CatalogSoftmaxLoss(nn.Module):
    """Cross-entropy of each user's ground-truth item against EVERY row of a resident catalogue (cosine scores / temperature), streamed
    in chunks by ``hip.catalog_softmax``: no sampled negatives, no [B,P,D] tensor, nothing of size B x N.  The catalogue is frozen; the
    gradient reaches the user embeddings only.
    ``matryoshka_dims`` (ascending multiples of 4 -- 8 for a bf16 catalogue -- the last one the embedding width) makes it the Matryoshka
    form, ``hip.catalog_mrl_softmax``: sum_k matryoshka_weights[k] * that loss on the first d_k components of the users and of every
    catalogue row, each prefix renormalised, the catalogue read in place; weights all ones unless given, a zero weight keeps the plane's
    loss in ``last_plane_loss`` and out of the sum and the gradient.  None is the plain loss: the same launches and bits as ever."""

    def __init__(self, catalog, temperature: float = 0.07, scorer=None, chunk_rows=None, matryoshka_dims=None, matryoshka_weights=None):
        """catalog: a CatalogEvaluator (its catalogue and cached norms are used where they lie), or an [N,D] f32 / bf16 device tensor.
        The catalogue's inverse norms are computed by the first call and kept -- with matryoshka_dims one plane per width, in the
        evaluator, where ``retrieve_funnel`` over the same widths finds them.  scorer, chunk_rows: as for CatalogEvaluator.retrieve."""
        super().__init__()
        from .evaluation import CatalogEvaluator
        hip.catalog_scorer_id(scorer)
        if not isinstance(catalog, CatalogEvaluator):
            catalog = torch.as_tensor(catalog)
            if catalog.dim() != 2 or catalog.dtype not in (F32, BF16):
                raise ValueError("CatalogSoftmaxLoss: catalog must be a CatalogEvaluator or an [N, D] f32 / bf16 tensor")
            catalog = CatalogEvaluator(catalog, device=catalog.device, dtype=catalog.dtype)
        if not float(temperature) > 0:
            raise ValueError(f"CatalogSoftmaxLoss: temperature must be positive, got {temperature}")
        self.evaluator, self.temperature, self.scorer, self.chunk_rows = catalog, float(temperature), scorer, chunk_rows
        if matryoshka_dims is None:
            if matryoshka_weights is not None:
                raise ValueError("matryoshka_weights needs matryoshka_dims")
            self.matryoshka_dims = self.matryoshka_weights = None
        else:
            D = catalog.catalog.shape[1]
            self.matryoshka_dims = hip.mrl_dims(matryoshka_dims, "matryoshka_dims", D)
            self.matryoshka_weights = hip.mrl_weights(matryoshka_weights, len(self.matryoshka_dims), "matryoshka_weights")
            if catalog.catalog.dtype == BF16 and any(d % 8 for d in self.matryoshka_dims):
                raise ValueError(f"matryoshka_dims: every entry must be a multiple of 8 for a bf16 catalogue, got {self.matryoshka_dims}")
        self.last_lse = self.last_row_loss = self.last_plane_loss = None
        self._planes = None

    @property
    def catalog(self):
        return self.evaluator.catalog

    def _norm_planes(self):
        """[K,N]: the evaluator's norm plane of every width (computed there once, shared with retrieve_funnel), stacked once"""
        if self._planes is None:
            by_dim = self.evaluator._prefix_norms(self.matryoshka_dims)
            self._planes = torch.stack([by_dim[d] for d in self.matryoshka_dims]).contiguous()
        return self._planes

    def forward(self, user_embeddings, positive_item_index, exclude=None):
        """exclude: the items each user has seen (ragged lists or [B,E] padded with -1); they leave the softmax's sum, except the user's
        own positive.  Keeps ``last_lse`` and ``last_row_loss`` [B] of the call; with matryoshka_dims they are [K,B], and
        ``last_plane_loss`` [K] holds the per-prefix losses."""
        from .evaluation import pack_exclude
        dev = self.catalog.device
        u = user_embeddings.contiguous().to(dev, F32)
        gt = torch.as_tensor(positive_item_index).to(dev, torch.int64)
        ex = pack_exclude(exclude, u.shape[0])
        ex = None if ex is None else ex.to(dev)
        if self.matryoshka_dims is not None:
            return _CatalogMrlSoftmaxFn.apply(u, self, gt, ex)
        return _CatalogSoftmaxFn.apply(u, self, gt, ex)


LOSSES = ("infonce", "catalog_softmax")
# batch keys that name or carry sampled candidates: a catalogue-softmax step has none
_CANDIDATE_KEYS = ("negative_item_index", "negative_masks", "positive_item_embeddings", "negative_item_embeddings")


class MultiModalTrainer:
    """compute_loss of the reference's HF-Trainer subclass (:477-498) without the Trainer."""

    def __init__(self, temperature: float = 0.07, negatives=None, loss: str = "infonce", matryoshka_dims=None, matryoshka_weights=None):
        """negatives: a ``negatives.CatalogCandidates``; needed by batches that carry ``positive_item_index`` instead of embeddings.
        loss: "infonce" (the reference's loss over one positive and the batch's negatives) or "catalog_softmax" (``CatalogSoftmaxLoss``
        over the whole catalogue of ``negatives``, which must then sample and mine nothing).
        matryoshka_dims, matryoshka_weights: the Matryoshka form of the loss (``InfoNCELoss``, ``CatalogSoftmaxLoss``): the loss on every
        nested prefix of the embeddings, for embedding batches and index batches alike.  Hard negatives are still mined with full-width
        scores: the mined set is the one the plain loss would train on, and every prefix is trained against it."""
        if loss not in LOSSES:
            raise ValueError(f"loss must be one of {LOSSES}, got {loss!r}")
        self.loss = loss
        self.infonce_loss = InfoNCELoss(temperature, matryoshka_dims, matryoshka_weights)
        self.negatives = negatives
        self.catalog_softmax_loss = None
        if loss == "catalog_softmax":
            if negatives is None:
                form = "" if matryoshka_dims is None else " with matryoshka_dims"
                raise ValueError(f'loss="catalog_softmax"{form} needs the `negatives` argument (a negatives.CatalogCandidates over the resident '
                                 "catalogue)")
            if negatives.num_random != 0 or negatives.num_hard != 0:
                raise ValueError(f'loss="catalog_softmax" sums over the whole catalogue: negatives.num_random and negatives.num_hard must be 0 '
                                 f"(got {negatives.num_random} and {negatives.num_hard})")
            if getattr(negatives, "coarse", False):
                raise ValueError('loss="catalog_softmax" has no coarse form (its gradient would need its own definition): '
                                 "negatives.coarse must be False")
            self.catalog_softmax_loss = CatalogSoftmaxLoss(negatives.evaluator, temperature, scorer=negatives.scorer,
                                                           chunk_rows=negatives.chunk_rows, matryoshka_dims=matryoshka_dims,
                                                           matryoshka_weights=matryoshka_weights)

    def compute_loss(self, model, inputs, return_outputs=False, step=0, **kwargs):
        """A batch with ``positive_item_index`` [B] takes its candidates from the resident catalogue of ``negatives``: optional
        ``negative_item_index`` [B,P] (padded with -1), ``negative_masks``, ``seen_item_index`` (ragged or [B,E] padded with -1), plus the
        random and mined negatives that object is configured for -- mined with the user embeddings of this very forward, random ones
        keyed on (step, global sample index).  Any other batch carries the embeddings themselves, as the reference's collator does.
        With loss="catalog_softmax" the batch holds ``positive_item_index`` and optionally ``seen_item_index`` and none of the
        candidate keys: every catalogue row the user has not seen is a candidate."""
        if self.loss == "catalog_softmax":
            if "positive_item_index" not in inputs:
                raise ValueError('compute_loss: loss="catalog_softmax" needs positive_item_index in the batch')
            for key in _CANDIDATE_KEYS:
                if key in inputs:
                    raise ValueError(f'compute_loss: loss="catalog_softmax" takes every catalogue row as a candidate; the batch must not '
                                     f"carry {key}")
        by_index = "positive_item_index" in inputs
        if by_index and self.negatives is None:
            raise ValueError("compute_loss: the batch holds positive_item_index, which needs the trainer's `negatives` argument "
                             "(a negatives.CatalogCandidates over the resident catalogue)")
        user_embeddings = model(input_ids=inputs["input_ids"], attention_mask=inputs["attention_mask"],
                                history_field_embeddings=inputs["history_field_embeddings"],
                                history_attention_mask=inputs["history_attention_mask"])
        if self.loss == "catalog_softmax":
            loss = self.catalog_softmax_loss(user_embeddings, inputs["positive_item_index"], exclude=inputs.get("seen_item_index", None))
        elif by_index:
            pos, neg, mask, _ = self.negatives.candidates(
                user_embeddings, inputs["positive_item_index"], inputs.get("negative_item_index", None), inputs.get("negative_masks", None),
                exclude=inputs.get("seen_item_index", None), step=step, first_sample=model.base_model.first_sample(user_embeddings.shape[0]))
            loss = self.infonce_loss(user_embeddings, pos, neg, mask)
        else:
            loss = self.infonce_loss(user_embeddings, inputs["positive_item_embeddings"], inputs["negative_item_embeddings"],
                                     inputs.get("negative_masks", None))
        return (loss, user_embeddings) if return_outputs else loss


# ---- the reference's optimisation step (HF Trainer with TrainingArguments, :755-773) -------------------------------------------------
# Trainer.get_decay_parameter_names: every parameter outside nn.LayerNorm modules whose dotted name (lower case) matches none of these
_NO_DECAY_PATTERNS = [re.compile(p) for p in (r"bias", r"layernorm", r"rmsnorm", r"(?:^|\.)norm(?:$|\.)", r"_norm(?:$|\.)")]


def decay_parameter_names(module):
    """Names of the parameters HF Trainer applies weight decay to (transformers' get_parameter_names(model, [nn.LayerNorm],
    patterns) rule, re-stated so the product path does not import transformers)."""
    out = []
    for name, child in module.named_children():
        out += [f"{name}.{n}" for n in decay_parameter_names(child)
                if not isinstance(child, nn.LayerNorm) and not any(p.search(f"{name}.{n}".lower()) for p in _NO_DECAY_PATTERNS)]
    out += [k for k in module._parameters if not any(p.search(k.lower()) for p in _NO_DECAY_PATTERNS)]
    return out


def no_decay_pack_names(model, packs):
    """Pack tensor names HF would step without weight decay (bias / LayerNorm / norm tensors), matched by parameter identity."""
    decay = set(decay_parameter_names(model))
    decay_ids = {id(p) for n, p in model.named_parameters() if n in decay}
    out, seen = set(), {}
    for pack in packs:
        for n in pack.names:
            exempt = id(pack.params[n]) not in decay_ids
            if seen.setdefault(n, exempt) != exempt:
                raise ValueError(f"{n}: one pack name with two weight-decay rules (FusedAdamW.no_decay is keyed on names)")
            if exempt:
                out.add(n)
    return out


class TrainingConfig:
    """What JointTrainer takes from a transformers.TrainingArguments (or any object with its attribute names)."""

    def __init__(self, args, num_training_steps=None):
        g = lambda name, dflt: dflt if getattr(args, name, None) is None else getattr(args, name)
        gas = int(g("gradient_accumulation_steps", 1))
        if gas != 1:
            raise ValueError(f"JointTrainer: gradient_accumulation_steps={gas} is not supported (one backward per optimizer step)")
        optim = str(getattr(g("optim", "adamw_torch"), "value", g("optim", "adamw_torch")))
        if not optim.startswith("adamw"):
            raise ValueError(f"JointTrainer: optim={optim!r}; the fused step is AdamW (torch.optim.AdamW semantics)")
        self.learning_rate = float(g("learning_rate", 5e-5))
        self.betas = (float(g("adam_beta1", 0.9)), float(g("adam_beta2", 0.999)))
        self.eps = float(g("adam_epsilon", 1e-8))
        self.weight_decay = float(g("weight_decay", 0.0))
        mgn = getattr(args, "max_grad_norm", 1.0)
        self.max_grad_norm = float(mgn) if mgn is not None and mgn > 0 else None      # HF: None or <= 0 turns clipping off
        self.lr_scheduler_type = str(getattr(g("lr_scheduler_type", "linear"), "value", g("lr_scheduler_type", "linear")))
        max_steps = g("max_steps", -1)
        self.num_training_steps = int(max_steps) if max_steps > 0 else (None if num_training_steps is None else int(num_training_steps))
        ws = g("warmup_steps", 0)
        if hasattr(args, "get_warmup_steps") and (self.num_training_steps is not None or ws >= 1 or ws == 0):
            self.warmup_steps = int(args.get_warmup_steps(self.num_training_steps if self.num_training_steps is not None else 0))
        elif ws >= 1 or ws == 0:
            self.warmup_steps = int(ws)
        else:
            raise ValueError("JointTrainer: a fractional warmup_steps needs max_steps or num_training_steps")
        ls = g("logging_steps", 500)
        if 0 < ls < 1:                  # HF: a ratio of the total steps
            if self.num_training_steps is None:
                raise ValueError("JointTrainer: a fractional logging_steps needs max_steps or num_training_steps")
            ls = math.ceil(self.num_training_steps * ls)
        self.logging_steps = int(ls)


class JointTrainerState:
    def __init__(self):
        self.global_step = 0
        self.log_history = []


class JointTrainer:
    """The step HF Trainer runs for the reference's joint model (:755-773) after ``compute_loss``, on the HIP path and nothing more
    (no dataloader, callbacks, evaluation loop or checkpoint directory -- DESIGN §8 keeps those with the caller):
    zero_grad -> MultiModalTrainer.compute_loss -> backward -> (bucket all-reduce waits) -> global gradient-norm clip + AdamW in
    one deterministic norm launch and the AdamW launches reading its coefficient on the device -> scheduler step.
    Under torch.distributed the gradient buckets are wired as bench.py wires them and 1/world is folded into the gradient scale:
    the norm is the norm of the averaged gradient (DDP + clip_grad_norm_), the same on every rank.  ``state.log_history`` gets
    {step, loss, grad_norm, learning_rate} every ``logging_steps`` -- the only host read (rank-local loss).
    ``negatives`` (a ``negatives.CatalogCandidates``) lets a batch name its candidates by index into a resident catalogue
    (``MultiModalTrainer.compute_loss``); the random negatives of such a batch are keyed on ``state.global_step``.
    ``loss="catalog_softmax"`` replaces InfoNCE by the softmax over that whole catalogue (``CatalogSoftmaxLoss``); gradient scale,
    clipping and logging are the same.  ``matryoshka_dims`` / ``matryoshka_weights`` make either loss its Matryoshka form
    (``InfoNCELoss``, ``CatalogSoftmaxLoss``); the log records then carry ``plane_loss``, the per-prefix losses averaged over the logging window."""

    def __init__(self, model, args, num_training_steps=None, temperature: float = 0.07, negatives=None, loss: str = "infonce",
                 matryoshka_dims=None, matryoshka_weights=None):
        from . import dp
        from .optim import FusedAdamW, get_scheduler
        # (first: a refused `loss` or `matryoshka_dims` touches neither model nor device)
        self.loss_fn = MultiModalTrainer(temperature, negatives, loss, matryoshka_dims, matryoshka_weights)
        self.model, self.args = model, args
        self.config = cfg = TrainingConfig(args, num_training_steps)
        dev = model.base_model.embed_tokens.weight.device
        qf, qw, uq = model.qformer_model, model.base_model, model.user_qformer
        self.qpack = None if qf is None else qf._ensure_pack(dev)
        self.lpack = qw._ensure_pack(dev)
        self.upack = None if uq is None else uq._ensure_pack(dev)
        self.packs = [p for p in (self.qpack, self.lpack, self.upack) if p is not None]
        self.no_decay = no_decay_pack_names(model, self.packs)
        self.optimizer = FusedAdamW(self.packs, lr=cfg.learning_rate, betas=cfg.betas, eps=cfg.eps, weight_decay=cfg.weight_decay,
                                    max_grad_norm=cfg.max_grad_norm, no_decay=self.no_decay if cfg.weight_decay > 0 else ())
        self.lr_scheduler = get_scheduler(cfg.lr_scheduler_type, self.optimizer, cfg.warmup_steps, cfg.num_training_steps)
        self.state = JointTrainerState()
        self._tr_loss, self._tr_planes, self._since_log = None, None, 0
        # data parallel: the buckets and hooks of bench.py's joint step (LoRA: groups of 7 layers; Q-Former: one bucket per layer)
        self.grad_scale, self.buckets, self.tail_buckets = 1.0, [], []
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
            dp.set_dp_rank(rank, model)
            self.grad_scale = 1.0 / world
            if self.lpack is not None:
                l_pre = [f"layers.{i}." for i in range(qw.config.num_hidden_layers)]
                lbk = dp.GradBuckets(self.lpack.grad, dp.layer_boundaries(self.lpack, l_pre, 7))
                qw.grad_ready_hook = dp.bucket_hook(self.lpack, lbk, l_pre, 7)
                self.buckets.append(lbk)
            if self.qpack is not None:
                q_pre = [f"qformer.encoder.layer.{i}." for i in range(qf.qformer.config.num_hidden_layers)]
                qbk = dp.GradBuckets(self.qpack.grad, dp.layer_boundaries(self.qpack, q_pre, 1))
                qf.qformer.grad_ready_hook = dp.bucket_hook(self.qpack, qbk, q_pre, 1)
                self.buckets.append(qbk)
            if self.upack is not None:
                self.tail_buckets.append(dp.GradBuckets(self.upack.grad, [0, self.upack.numel]))

    def compute_loss(self, model, inputs, return_outputs=False, **kwargs):
        kwargs.setdefault("step", self.state.global_step)       # keys the random negatives of an index batch
        return self.loss_fn.compute_loss(model, inputs, return_outputs=return_outputs, **kwargs)

    def training_step(self, inputs):
        """One optimizer step on `inputs` (the batch dict of the reference's collator); returns the loss as a device tensor."""
        opt = self.optimizer
        self.model.train()
        opt.zero_grad()
        loss = self.compute_loss(self.model, inputs)
        loss.backward()
        for bk in self.tail_buckets:
            bk.ready_all()
        for bk in self.tail_buckets + self.buckets:
            bk.wait()
        lr = opt.lr                       # the scheduled rate of this step (HF logs it before the scheduler moves on)
        opt.step(grad_scale=self.grad_scale)
        self.lr_scheduler.step()
        self.state.global_step += 1
        loss = loss.detach()
        self._tr_loss = loss.clone() if self._tr_loss is None else self._tr_loss + loss
        planes = (self.loss_fn.infonce_loss if self.loss_fn.loss == "infonce" else self.loss_fn.catalog_softmax_loss).last_plane_loss
        if planes is not None:
            self._tr_planes = planes.clone() if self._tr_planes is None else self._tr_planes + planes
        self._since_log += 1
        ls = self.config.logging_steps
        if ls > 0 and self.state.global_step % ls == 0:
            self._log(lr)
        return loss

    def _log(self, lr):
        vals = [self._tr_loss.float()]
        norm = self.optimizer.last_grad_norm
        if norm is not None:
            vals.append(norm)
        planes = self._tr_planes
        host = torch.cat([torch.stack(vals)] + ([] if planes is None else [planes.float()])).tolist()      # the one host read
        rec = {"step": self.state.global_step, "loss": host[0] / self._since_log}
        if norm is not None:
            rec["grad_norm"] = host[1]
        rec["learning_rate"] = lr
        if planes is not None:
            rec["plane_loss"] = [v / self._since_log for v in host[len(vals):]]
        self.state.log_history.append(rec)
        self._tr_loss, self._tr_planes, self._since_log = None, None, 0
