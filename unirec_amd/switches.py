"""The A/B switches of the decoder and the Q-Formers: the ONE place the product path reads the environment for them.

`switches` is built once, when the package is imported; setting a UNIREC_* variable afterwards has no effect.  The defaults are the
product path; every other value selects a complete alternative launch sequence kept for the parity tests and for same-box A/B
timing (README "Switches").  Tests flip a field with ``monkeypatch.setattr(switches, field, value)``.
"""
import os
from dataclasses import dataclass, fields
from typing import Optional


@dataclass
class Switches:
    # ---- decoder (qwen3.py) ----
    # UNIREC_MERGE_PROJ=0 (lab): one projection launch per LoRA adapter instead of the merged q|k|v and gate|up launches
    merge_proj: bool = True
    # UNIREC_FUSE_NORM_LORA=0 (lab): RMSNorm forward and the q|k|v / gate|up adapters' down projection as two kernels again
    fuse_norm_lora: bool = True
    # UNIREC_FUSE_QK_ROPE=0 (lab): q/k-norm + RoPE as their own pass over the raw q|k|v again (the fused form needs the persistent GEMM:
    # >= 128 output tiles, S >= 256, head_dim 128; smaller launches take the separate pass anyway)
    fuse_qk_rope: bool = True
    # UNIREC_FUSE_SWIGLU_GEMM=0 (lab): SwiGLU forward as its own pass over gate|up again (the fused form rides in the merged gate|up launch on
    # the persistent GEMM: interleaved weight rows put gate and up of a feature into one lane; the down adapter's t = dropout(act) A^T is
    # then a lora_project pass over act)
    fuse_swiglu_gemm: bool = True
    # UNIREC_FUSE_SWIGLU_LORA=0 (lab): SwiGLU forward and the down_proj adapter's down projection as two kernels again
    fuse_swiglu_lora: bool = True
    # UNIREC_SWIGLU_FWD_FUSED=1 runs SwiGLU forward as the up projection's epilogue (ur_gemm swiglu_gate) instead of its own launch.
    # Measured neutral on the joint step (115.1 vs 115.5 seq/s on one box, alternating runs: the epilogue's extra gate read and act
    # write are not overlapped with MFMA work at one workgroup per CU, and the stand-alone kernel already streams at 5.4 TB/s), so
    # the separate launch stays the default; the backward fusion (swiglu_gu), which removes 6 of 15 activation passes, is always on.
    # (Needs the per-adapter launches: it has no effect unless UNIREC_MERGE_PROJ=0 as well.)
    swiglu_fwd_fused: bool = False
    # UNIREC_RECOMPUTE_MLP=1: the default of Qwen3LoRAModel.recompute_mlp (drop gate|up and act after the forward, rebuild them in the backward)
    recompute_mlp: bool = False
    # UNIREC_BITS_ONE_EVENT=1 (lab): wait for every layer's prefetched dropout planes before the first layer, the former behaviour
    bits_one_event: bool = False
    # UNIREC_BITS_T=0 (lab): no token-packed copies of the dropout flags, lora_reduce runs its register-staged reduction
    bits_t: bool = True
    # UNIREC_BITS_NEXT=0 (lab): the backward does not regenerate the flag planes for the following step; every step makes its own at its start
    bits_next: bool = True
    # UNIREC_PAD_ATT=0 (lab): attention output rows unpadded (a power-of-two row stride)
    pad_att: bool = True
    # UNIREC_ROPE_K_FUSED=0 (test / lab): the k heads' q/k-norm + RoPE backward by a separate launch instead of the dK/dV kernel's store
    rope_k_fused: bool = True
    # UNIREC_ROPE_BWD_FUSED, three-valued: does the q heads' q/k-norm + RoPE backward ride in the dQ kernel's store?
    #   None (unset): yes from the roped outputs (the forward fused q/k-norm + RoPE into the q|k|v launch), no from the raw projection
    #   True ("1"):   yes in both cases.  From the raw projection it is parity-tested and measured neutral on the joint step (115.7 vs
    #                 115.9 seq/s, alternating same-box runs: the ~1000 vector instructions per wave in the dQ kernel's store cost what
    #                 the 4 saved activation passes return), so the separate launch stays the default there.
    #   False ("0"):  no in both cases (the stand-alone kernels)
    rope_bwd_fused: Optional[bool] = None
    # ---- Q-Formers (qformer.py) ----
    # UNIREC_KV_COLSUM=0 (test / lab): the K | V bias gradients by a column-sum pass over dK | dV again
    kv_colsum: bool = True
    # UNIREC_QF_WT=0 (lab): dX products read the [out, in] weights as K-strided operands again
    qf_wt: bool = True
    # UNIREC_QF_DW_STREAM: round 6: the weight gradients dW = dY^T X (token reductions, split-K) and the bias column sums of the backward are
    # issued on a SIDE stream: they hang off the dX chain (nothing in the backward reads them) and neither they nor the dX products fill
    # 256 CUs at the Q-Formers' row counts (item Q-Former of the joint step: 6400 rows = 100 output tiles), so the two streams' kernels
    # run beside each other.  Same kernels, same arithmetic: results bit-identical (tests/test_gpu_r6_parity.py).
    # 0 = everything on the caller's stream, as before.
    qf_dw_stream: bool = True
    # UNIREC_QF_DW_GROUPED=0: one ur_gemm per weight gradient of a Q-Former layer instead of the layer's ur_gemm_grouped launch
    qf_dw_grouped: bool = True

    @classmethod
    def variables(cls):
        """field name -> environment variable"""
        return {f.name: "UNIREC_" + f.name.upper() for f in fields(cls)}

    @classmethod
    def from_env(cls, env):
        """The switches a mapping of environment variables selects (pure: reads nothing but `env`).  A field that defaults to on is
        on unless its variable is "0", one that defaults to off is off unless it is "1"; rope_bwd_fused is None unless "0" / "1"."""
        return cls(**{f.name: {"0": False, "1": True}.get(env.get("UNIREC_" + f.name.upper()), f.default) for f in fields(cls)})


switches = Switches.from_env(os.environ)
