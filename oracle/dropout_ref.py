"""Counter-based dropout keep masks, restated in numpy (TEST INFRASTRUCTURE ONLY).

The HIP kernels never store a dropout mask: every site regenerates ``keep = hash(seed, element counter) >= p * 2^32`` in the
forward and in the backward (unirec_amd/csrc/common.hip.h: ur_hash2 / ur_dropout_scale / ur_drop_threshold).  This module restates
that generator (and the pair-word form the attention kernels use: attn_keep_rows) and the counter layouts so that

  * the golden generator (tests/golden/make_golden_r5.py) can make the REFERENCE's nn.Dropout modules
    (/root/reference/models/qformer.py:66,107 embeddings; :135,258 attention probabilities; :283,287 BertSelfOutput; :369,373
    BertOutput) apply exactly the masks the kernels draw, and
  * the parity tests can feed the same masks to the training-mode oracle (oracle/qformer_train_ref.py).

`ur_dropout_keep` / `ur_attn_dropout_keep` (include/unirec_hip.h) export the device-side flags; a GPU test checks them against this
file bit for bit.
"""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def _u32(x):
    return np.asarray(x, dtype=np.uint64) & _M32


def hash2(seed, idx):
    """32-bit decision word of element `idx` (uint64 array) of stream `seed` -- common.hip.h: ur_hash2."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s0, s1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    rot = _u32((s1 << np.uint64(13)) | (s1 >> np.uint64(19)))
    k2 = _u32(s0 * np.uint64(0x7FEB352D)) ^ rot ^ np.uint64(0x5851F42D)
    idx = np.asarray(idx, dtype=np.uint64)
    lo, hi = idx & _M32, idx >> np.uint64(32)
    h = _u32(_u32((lo ^ s0) * np.uint64(0x9E3779B1)) + _u32(hi + s1))
    h ^= h >> np.uint64(16)
    h = _u32(h * np.uint64(0x85EBCA6B))
    h ^= k2
    h ^= h >> np.uint64(13)
    h = _u32(h * np.uint64(0xC2B2AE35))
    h ^= h >> np.uint64(16)
    return h


def threshold(p):
    """p * 2^32 as the kernels compute it (the float p widened to double, truncated, clamped) -- common.hip.h: ur_drop_threshold."""
    t = float(np.float32(p)) * 4294967296.0
    return np.uint64(int(min(max(t, 0.0), 4294967295.0)))


def keep_range(seed, p, idx0, n):
    """uint8 [n]: keep flags of counters idx0 .. idx0 + n - 1."""
    idx = np.uint64(int(idx0)) + np.arange(int(n), dtype=np.uint64)
    return (hash2(seed, idx) >= threshold(p)).astype(np.uint8)


def hidden_keep(seed, p, rows, H, row0=0):
    """[rows, H] keep mask of a hidden-dropout site: counter = (row0 + row) * H + column (norm.hip: make_drop)."""
    return keep_range(seed, p, int(row0) * int(H), int(rows) * int(H)).reshape(int(rows), int(H))


def threshold16(p):
    """p * 65536 rounded, at least 1 for p > 0 -- common.hip.h: ur_drop_threshold16 as attn.hip uses it."""
    if p <= 0:
        return np.uint64(0)
    t = float(np.float32(p)) * 65536.0 + 0.5
    return np.uint64(max(1, int(min(max(t, 0.0), 65535.0))))


def attn_row_keys(seed, rows):
    """the two 32-bit keys of dropout rows `rows` (uint64 array) -- common.hip.h: ur_attn_row_key"""
    rows = np.asarray(rows, dtype=np.uint64)
    return hash2(seed, rows * np.uint64(2)), hash2(seed, rows * np.uint64(2) + np.uint64(1))


def attn_pair_word(k1, k2, kp):
    """decision word of key pair kp of a row with keys (k1, k2) -- common.hip.h: ur_attn_pair_word (a two-multiply finaliser over
    kp ^ k1 with k2 added between the rounds)"""
    x = _u32(np.asarray(kp, dtype=np.uint64) ^ k1)
    x ^= x >> np.uint64(16)
    x = _u32(x * np.uint64(0x7FEB352D))
    x = _u32(x + k2)
    x ^= x >> np.uint64(15)
    x = _u32(x * np.uint64(0x846CA68B))
    x ^= x >> np.uint64(16)
    return x


def attn_keep_rows(seed, p, row0, nrows, Sk):
    """uint8 [nrows, Sk]: keep flags of dropout rows row0 .. row0 + nrows - 1 (one 32-bit word per PAIR of keys: its low / high
    16 bits decide keys 2 kp / 2 kp + 1 against p * 65536) -- what ur_attn_dropout_keep exports."""
    rows = np.uint64(int(row0)) + np.arange(int(nrows), dtype=np.uint64)
    k1, k2 = attn_row_keys(seed, rows)
    kp = np.arange((int(Sk) + 1) // 2, dtype=np.uint64)
    w = attn_pair_word(k1[:, None], k2[:, None], kp[None, :])
    fields = np.stack([w & np.uint64(0xFFFF), w >> np.uint64(16)], -1).reshape(int(nrows), -1)[:, :int(Sk)]
    return (fields >= threshold16(p)).astype(np.uint8)


def attn_keep(seed, p, B, nh, Sq, Sk, b0=0):
    """[B, nh, Sq, Sk] keep mask of an attention-probability site: dropout row of (b, h, q) = ((b0 + b) * nh + h) * Sq + q
    (attn.hip: AttnP.drow0)."""
    return attn_keep_rows(seed, p, int(b0) * int(nh) * int(Sq), int(B) * int(nh) * int(Sq), Sk).reshape(int(B), int(nh), int(Sq), int(Sk))


# dropout sites of one Q-Former layer, in the product's numbering (unirec_amd/qformer.py:_layer_forward); the embeddings site is
# (layer 1023, site 0)
SITE_SELF_PROBS, SITE_SELF_OUT, SITE_CROSS_PROBS, SITE_CROSS_OUT, SITE_FFN_OUT = 1, 2, 3, 4, 5
EMB_LAYER, EMB_SITE = 1023, 0


def site_seed(base_seed, step, layer, site):
    """Seed of one dropout site of one step (unirec_amd/qformer.py: BertModel._seed) -- restated here so that fixtures do not
    depend on the product code; a GPU test asserts the two agree."""
    return (int(base_seed) * 1000003 + int(step) * 8191 + int(layer) * 64 + int(site)) & 0x7FFFFFFFFFFFFFFF


def qformer_masks(base_seed, step, p, B, Q, T, H, nh, num_layers, cross_freq, b0=0):
    """Every keep mask of one training-mode Q-Former forward, keyed as oracle/qformer_train_ref.py expects them."""
    m = {"emb": hidden_keep(site_seed(base_seed, step, EMB_LAYER, EMB_SITE), p, B * Q, H, b0 * Q).reshape(B, Q, H)}
    for i in range(num_layers):
        s = lambda site: site_seed(base_seed, step, i, site)
        m[f"{i}.self.probs"] = attn_keep(s(SITE_SELF_PROBS), p, B, nh, Q, Q, b0)
        m[f"{i}.self.out"] = hidden_keep(s(SITE_SELF_OUT), p, B * Q, H, b0 * Q).reshape(B, Q, H)
        if i % cross_freq == 0:
            m[f"{i}.cross.probs"] = attn_keep(s(SITE_CROSS_PROBS), p, B, nh, Q, T, b0)
            m[f"{i}.cross.out"] = hidden_keep(s(SITE_CROSS_OUT), p, B * Q, H, b0 * Q).reshape(B, Q, H)
        m[f"{i}.ffn.out"] = hidden_keep(s(SITE_FFN_OUT), p, B * Q, H, b0 * Q).reshape(B, Q, H)
    return m


# ---- LoRA dropped-flag bit planes (unirec_amd/csrc/lora.hip: header comment, lora_bits_kernel, ur_lora_dropout_bits) ----------------
# One 32-bit word per (adapter plane a, row m, group q of 32 columns); the row of a plane is lora_bits_ld(W) bytes = ng words, the words
# whose 32 columns all lie at or past W are zero.  Every element draws a 15-bit value u and is DROPPED iff u < thr15.
_PAIR_ELEM = np.array([0, 2, 4, 6, 1, 3, 5, 7])         # bit i of a flag byte -> element of its 8 columns (i < 4: c + 2i, 4 + i: c + 2i + 1)
_LORA_GOLD = np.uint64(0x9E3779B9)


def lora_bits_ld(W):
    """bytes per row of a bit plane: 16 per 128 columns (ur_lora_bits_ld)"""
    return (int(W) + 127) // 128 * 16


def lora_thr15(p):
    """p * 2^15 rounded to nearest (the float p widened to double, + 0.5, truncated), clamped to 32767 -- ur_lora_dropout_bits"""
    t = float(np.float32(p)) * 32768.0 + 0.5
    return 32767 if t > 32767.0 else int(t)


def _fmix32(h):
    h = _u32(h)
    h ^= h >> np.uint64(16)
    h = _u32(h * np.uint64(0x85EBCA6B))
    h ^= h >> np.uint64(13)
    h = _u32(h * np.uint64(0xC2B2AE35))
    h ^= h >> np.uint64(16)
    return h


def _lora_round(w):
    """one multiply-xorshift round of the chain"""
    w = w ^ (w >> np.uint64(16))
    w = _u32(w * np.uint64(0x7FEB352D))
    return w ^ (w >> np.uint64(15))


def lora_word_keys(seed, M, W, nad, row0=0):
    """uint64 [nad, M, ng]: the never-zero start state of every word's chain -- the 64-bit counter ((row0 + m) * ng + q) << 2 | a,
    murmur-finalised with the seed and the seed-only key k2 entered before and after the last round."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s_lo, s_hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    rot = _u32((s_hi << np.uint64(13)) | (s_hi >> np.uint64(19)))
    k2 = _fmix32(_u32(s_lo * np.uint64(0x7FEB352D)) ^ rot ^ np.uint64(0x5851F42D))
    ng = lora_bits_ld(W) // 4
    with np.errstate(over="ignore"):
        rows = np.asarray([int(row0) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64) + np.arange(int(M), dtype=np.uint64)
        ctr = ((rows[None, :, None] * np.uint64(ng) + np.arange(ng, dtype=np.uint64)[None, None, :]) << np.uint64(2)) \
            + np.arange(int(nad), dtype=np.uint64)[:, None, None]
    lo, hi = ctr & _M32, ctr >> np.uint64(32)
    h = _u32(_fmix32(_u32((lo ^ s_lo) + _fmix32(hi + s_hi + _LORA_GOLD)) ^ k2) + k2)
    return np.where(h == 0, _LORA_GOLD, h)


def lora_words(seed, p, M, W, nad, row0=0):
    """uint32 [nad, M, lora_bits_ld(W) / 4]: the dropped-flag words ur_lora_dropout_bits writes (little-endian: byte c / 8 of a row covers
    columns c .. c + 7).  Bit-sliced: state k of the chain carries bit k of the word's 32 values, from thr15's lowest set bit k0 up to
    bit 14, and lt_k = t_k ? (~b_k | lt_{k-1}) : (~b_k & lt_{k-1}) is the comparison u < thr15 restricted to the bits k0 .. k."""
    thr = lora_thr15(p)
    w = lora_word_keys(seed, M, W, nad, row0)
    lt = np.zeros_like(w)
    if thr != 0:
        k0 = (thr & -thr).bit_length() - 1
        tb = (thr >> k0) | (0x8000 >> k0)                # the sentinel above bit 14: thr's zero bits above its top bit count
        while tb != 1:
            w = _lora_round(w)
            nw = ~w & _M32
            lt = ((nw | lt) if tb & 1 else (nw & lt))
            tb >>= 1
    ng = w.shape[-1]
    live = (np.arange(ng) * 32 < int(W))[None, None, :]
    return np.where(live, lt, np.uint64(0)).astype(np.uint32)


def lora_dropped_plain(seed, p, M, W, nad, row0=0):
    """uint8 [nad, M, W]: the same flags element by element -- bit b of the word is the flag of column 32 q + 8 (b / 8) + PAIR[b % 8]; its
    15-bit value u takes bit k (k0 <= k <= 14) from bit b of chain state k - k0 + 1 and zeros below k0 (thr15 has zeros there, so those
    bits cannot decide); dropped iff u < thr15."""
    thr = lora_thr15(p)
    w = lora_word_keys(seed, M, W, nad, row0)
    ng = w.shape[-1]
    out = np.zeros((int(nad), int(M), ng * 32), dtype=np.uint8)
    if thr != 0:
        k0 = (thr & -thr).bit_length() - 1
        u = np.zeros(w.shape + (32,), dtype=np.int64)
        b = np.arange(32, dtype=np.uint64)
        for k in range(k0, 15):
            w = _lora_round(w)
            u |= (((w[..., None] >> b) & np.uint64(1)).astype(np.int64)) << k
        col = 8 * (np.arange(32) // 8) + _PAIR_ELEM[np.arange(32) % 8]               # column of bit b inside the word
        flags = (u < thr).astype(np.uint8)                                          # [nad, M, ng, 32] indexed by bit
        out.reshape(int(nad), int(M), ng, 32)[..., col] = flags
    return out[:, :, :int(W)]


def lora_keep(seed, p, M, W, nad, row0=0):
    """uint8 [nad, M, W] keep flags (1 = kept), unpacked from lora_words here: element e of byte c / 8 sits at bit e / 2 + 4 (e % 2)."""
    words = lora_words(seed, p, M, W, nad, row0).astype(np.uint64)
    c = np.arange(int(W))
    e = c % 8
    shift = (8 * ((c % 32) // 8) + e // 2 + 4 * (e % 2)).astype(np.uint64)
    dropped = (words[:, :, c // 32] >> shift[None, None, :]) & np.uint64(1)
    return (1 - dropped).astype(np.uint8)


def lora_words_transposed(words, W):
    """uint32 [nad, M / 32, (W + 3) / 4 * 4]: the token-packed repack ur_lora_bits_transpose makes of the planes (M % 32 == 0): word
    (group tg, column c) carries the flags of tokens 32 tg .. + 31 of column c, token t at bit 8 (t / 8) + (t % 8) / 2 + 4 (t % 2) (the
    pair order again, over tokens); the columns W .. ld - 1 carry whatever the row words hold there."""
    words = np.asarray(words).astype(np.uint64)
    nad, M, ng = words.shape
    assert M % 32 == 0
    ldt = (int(W) + 3) // 4 * 4
    c = np.arange(ldt)
    e = c % 8
    shift = (8 * ((c % 32) // 8) + e // 2 + 4 * (e % 2)).astype(np.uint64)
    dropped = ((words[:, :, c // 32] >> shift[None, None, :]) & np.uint64(1)).reshape(nad, M // 32, 32, ldt)
    t = np.arange(32)
    tpos = (8 * (t // 8) + (t % 8) // 2 + 4 * (t % 2)).astype(np.uint64)
    return (dropped << tpos[None, None, :, None]).sum(axis=2).astype(np.uint32)
