"""Host side of the autoregressive speech-token decoder (talker + code predictor) over libqtts.

`TalkerEngine.generate` mirrors the seam S2 of the reference:
`self.talker.generate(inputs_embeds, attention_mask, trailing_text_hidden, tts_pad_embed, **talker_kwargs)`
(qwen_tts/core/models/modeling_qwen3_tts.py:2272-2278), i.e. HF `_sample` around
Qwen3TTSTalkerForConditionalGeneration.forward (M:1636-1744).  All arithmetic runs in the HIP library.
"""
import ctypes as C
import threading
from dataclasses import dataclass
from typing import Any, Dict, List, Optional

import torch

from . import _lib
from .config import TalkerConfig
from .refill import RefillPacket, RefillPolicy, RefillRow, widest_opener


def _default_inv_freq(theta: float, head_dim: int) -> torch.Tensor:
    """HF 'default' rope init exactly as the reference's rotary modules compute it (M:538-541, 573-576)."""
    return 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).to(dtype=torch.float) / head_dim))


def _fresh_seed() -> int:
    """Default Philox seed of a sampling call: drawn from torch's ADVANCING default generator, so that two calls give two
    takes (as the reference's torch.multinomial does) while `torch.manual_seed(s)` still makes a run reproducible."""
    return int(torch.randint(0, 2 ** 62, (), dtype=torch.int64).item())


@dataclass
class TalkerGenerateOutput:
    codes: torch.Tensor        # (B, n_frames, G) int64, untrimmed (M:2280)
    hidden: Optional[torch.Tensor]  # (B, n_frames, H) float32 `past_hidden` per frame (M:2281)
    tokens: torch.Tensor       # (B, n_tokens) int64 sampled codebook-0 tokens (HF `sequences`)
    n_frames: int
    own: Optional[torch.Tensor] = None           # teacher forcing only: (B, F + 1, G) int32, the engine's OWN greedy choices
    logits_trace: Optional[torch.Tensor] = None  # teacher forcing only: (n_steps, B, vocab) raw cb-0 logits of `logit_steps`


@dataclass
class _Call:
    """A generation call as `TalkerEngine._prepare` hands it to `generate`, `generate_stream` and the refill schedules: checked, on the
    device, settings resolved.  Exactly one of `rows` (the per-row table; `warp` and `proc` may come with it) and `sp` (the scalar path) is set."""
    B: int
    T: int
    n_pad: List[int]
    lens: List[int]            # T - n_pad
    emb: torch.Tensor          # (B, T, H) fp32 on the device, contiguous (as `trail` (B, Tt, H) and `pad` (H,))
    trail: torch.Tensor
    pad: torch.Tensor
    eos: int
    suppress: List[int]
    npad_c: Any                # n_pad and suppress as the C ABI takes them
    sup_c: Any
    rows: Any                  # `_lib.RowSamplingC` x B, or None
    warp: Any                  # `_lib.RowWarpersC` x B, or None
    proc: Any                  # `_lib.RowProcessorsC` x B, or None
    sp: Any                    # `_lib.SamplingC`, or None
    max_new_tokens: int        # clamped to the KV capacity; on the table the largest limit (buffers are sized by it)
    min_new_tokens: Any        # as given (the scalar path passes it on; the table holds its own)


_SKIP_PREFIXES = ("speaker_encoder.",)


def _as_index(v):
    """An integer-like scalar (int, numpy / torch integer) as int, else None (bool is not an index here)."""
    import operator
    if isinstance(v, bool):
        return None
    try:
        return operator.index(v)
    except TypeError:
        return None


def _check_warpers(**kw):
    """HF's own argument checks (transformers generation/logits_process.py: TopKLogitsWarper / TopPLogitsWarper /
    TemperatureLogitsWarper constructors), so that a bad value fails like the reference instead of reaching the kernel.
    `top_p` follows HF literally: only values < 0 or > 1 raise; `top_p == 0` is legal there (the sorted cumulative mass cut removes
    everything and `min_tokens_to_keep = 1` puts the top token back) and is run here as `top_k = 1` (`_resolve_top`).  Integer-like
    scalars (numpy / torch integers) are accepted for `top_k`, which is more lenient than HF's `isinstance(top_k, int)`."""
    for name in ("top_k", "subtalker_top_k"):
        v = kw.get(name)
        if v is not None and v != 0 and (_as_index(v) is None or _as_index(v) < 0):
            raise ValueError(f"`{name}` has to be a strictly positive integer, but is {v}")
    for name in ("top_p", "subtalker_top_p"):
        v = kw.get(name)
        if v is not None and not (0.0 <= float(v) <= 1.0):
            raise ValueError(f"`{name}` has to be a float > 0 and < 1, but is {v}")
    for name in ("temperature", "subtalker_temperature"):
        v = kw.get(name)
        if v is not None and not float(v) > 0.0:
            raise ValueError(f"`{name}` (={v}) has to be a strictly positive float")


def _resolve_top(top_k, top_p):
    """(top_k, top_p) as the kernel takes them: `top_p == 0` keeps exactly the top token under HF's rule (see `_check_warpers`),
    which is `top_k = 1` with no nucleus cut."""
    k = _as_index(top_k) if top_k else 0
    p = float(top_p) if top_p is not None else 1.0
    if p == 0.0:
        return 1, 1.0
    return int(k or 0), p


_ROW_ARGS = ("do_sample", "top_k", "top_p", "temperature", "repetition_penalty", "subtalker_dosample", "subtalker_top_k",
             "subtalker_top_p", "subtalker_temperature", "max_new_tokens", "min_new_tokens", "seed")


def _fill_sampling(e, r):
    """The sampling knobs and the seed of a call (`_lib.SamplingC`) or of one request (`_lib.RowSamplingC`), which name them alike, from
    the values `r` (a dict over `_ROW_ARGS`), checked as HF checks them.  No seed draws a fresh one."""
    _check_warpers(**{k: r[k] for k in ("top_k", "top_p", "temperature", "subtalker_top_k", "subtalker_top_p", "subtalker_temperature")})
    e.do_sample = 1 if r["do_sample"] else 0
    e.top_k, e.top_p = _resolve_top(r["top_k"], r["top_p"])
    e.temperature = float(r["temperature"]) if r["temperature"] is not None else 1.0
    e.repetition_penalty = float(r["repetition_penalty"]) if r["repetition_penalty"] is not None else 1.0
    e.subtalker_dosample = 1 if r["subtalker_dosample"] else 0
    e.subtalker_top_k, e.subtalker_top_p = _resolve_top(r["subtalker_top_k"], r["subtalker_top_p"])
    e.subtalker_temperature = float(r["subtalker_temperature"]) if r["subtalker_temperature"] is not None else 1.0
    e.seed = int(r["seed"]) & 0xFFFFFFFFFFFFFFFF if r["seed"] is not None else _fresh_seed()


# the talker's remaining HF sampling controls (include/qtts.h `qtts_row_warpers`): per request like the knobs above, always on the table
_WARP_ARGS = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff", "no_repeat_ngram_size")


def _resolve_row_warpers(min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None, no_repeat_ngram_size=None):
    """One request's (min_p, typical_p, epsilon_cutoff, eta_cutoff, no_repeat_ngram_size) as the kernel takes them, 0 = off.  Gating is
    transformers' `_get_logits_processor`: `min_p` None or 0 is off, `typical_p` None or >= 1 is off, the cutoffs act only for
    0 < v < 1, `no_repeat_ngram_size` None or <= 0 is off.  Values HF's constructors refuse raise with HF's wording."""
    mp = 0.0
    if min_p is not None and min_p != 0:
        mp = float(min_p)
        if not 0.0 <= mp <= 1.0:
            raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {min_p}")
    tp = 0.0
    if typical_p is not None and float(typical_p) < 1.0:
        tp = float(typical_p)
        if not tp > 0.0:
            raise ValueError(f"`typical_p` has to be a float > 0 and < 1, but is {typical_p}")
    cut = [float(v) if v is not None and 0.0 < float(v) < 1.0 else 0.0 for v in (epsilon_cutoff, eta_cutoff)]
    n = 0
    if no_repeat_ngram_size is not None:
        n = _as_index(no_repeat_ngram_size)
        if n is None:
            raise ValueError(f"`ngram_size` has to be a strictly positive integer, but is {no_repeat_ngram_size}")
        n = max(0, n)
    return mp, tp, cut[0], cut[1], n


def _warp_table(B: int, **kw):
    """The warper table of a call (`_lib.RowWarpersC` x B) from the five `_WARP_ARGS`, each one value or a sequence of B; None when no
    request has any of them on (the call is then exactly the call without them)."""
    cols = {}
    for k in _WARP_ARGS:
        v = kw.get(k)
        if _is_row_seq(v):
            v = [_scalar(x) for x in v]
            if len(v) != B:
                raise ValueError(f"`{k}` has {len(v)} entries for a batch of {B} requests")
        else:
            v = [v] * B
        cols[k] = v
    rows = (_lib.RowWarpersC * B)()
    on = False
    for b in range(B):
        vals = _resolve_row_warpers(**{k: cols[k][b] for k in _WARP_ARGS})
        e = rows[b]
        e.min_p, e.typical_p, e.epsilon_cutoff, e.eta_cutoff, e.no_repeat_ngram_size = vals
        on = on or any(vals)
    return rows if on else None


# the talker's remaining HF logits processors (include/qtts.h `qtts_row_processors`; `min_length` is folded into the row's EOS floor)
_PROC_ARGS = ("sequence_bias", "bad_words_ids", "min_length", "forced_eos_token_id", "exponential_decay_length_penalty",
              "begin_suppress_tokens")


def _is_num(v) -> bool:
    return v is not None and not isinstance(v, (list, tuple, dict, str))


def _is_ids(v) -> bool:
    return isinstance(v, (list, tuple)) and all(_is_num(x) for x in v)


# HF's own form of each value: such a value is ONE value for the call
_PROC_IS_VALUE = {
    "sequence_bias": lambda v: isinstance(v, dict) or (isinstance(v, list) and all(
        isinstance(x, (list, tuple)) and len(x) == 2 and _is_ids(x[0]) and _is_num(x[1]) for x in v)),
    "bad_words_ids": lambda v: isinstance(v, list) and all(_is_ids(x) for x in v),
    "min_length": _is_num,
    "forced_eos_token_id": _is_num,
    "exponential_decay_length_penalty": lambda v: isinstance(v, (list, tuple)) and len(v) == 2 and _is_num(v[0]) and _is_num(v[1]),
    "begin_suppress_tokens": _is_ids,
}


def _split_row_processors(B: int, **kw) -> Dict[str, list]:
    """Which of the `_PROC_ARGS` values are shared and which are per request -- the one rule, used by every entry: HF's own form of a
    value is one value for the call; a list of length B whose items are each None (off for that request) or such a value is per
    request; a list of such items of any other length raises, naming the argument.  (`forced_eos_token_id`: a list is therefore always
    per request.)  Anything else is passed on as one value, for `_resolve_row_processors` to refuse in HF's wording.  Returns
    {name: list of B values}, for the names that are given."""
    out = {}
    for k in _PROC_ARGS:
        v = kw.get(k)
        if v is None:
            continue
        if not _PROC_IS_VALUE[k](v) and isinstance(v, (list, tuple)) and all(x is None or _PROC_IS_VALUE[k](x) for x in v):
            if len(v) != B:
                raise ValueError(f"`{k}` has {len(v)} entries for a batch of {B} requests")
            out[k] = list(v)
        else:
            out[k] = [v] * B
    return out


def _sequence_bias_dict(sequence_bias) -> dict:
    """SequenceBiasLogitsProcessor's `_validate_arguments` and `_convert_list_arguments_into_dict`, in HF's wording."""
    import numbers
    sb = sequence_bias
    is_id = lambda t: isinstance(t, numbers.Integral) and not isinstance(t, bool)
    if (not isinstance(sb, dict) and not isinstance(sb, list)) or len(sb) == 0:
        raise ValueError(f"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is {sb}.")
    if isinstance(sb, dict):
        if any(not isinstance(ids, tuple) for ids in sb):
            raise ValueError(f"`sequence_bias` has to be a dict with tuples as keys, but is {sb}.")
        if any(any((not is_id(t) or t < 0) for t in ids) or len(ids) == 0 for ids in sb):
            raise ValueError(f"Each key in `sequence_bias` has to be a non-empty tuple of positive integers, but is {sb}.")
        if any(not isinstance(b, float) for b in sb.values()):
            raise ValueError(f"`sequence_bias` has to be a dict with floats as values, but is {sb}.")
        return dict(sb)
    ok = lambda s: (isinstance(s, (list, tuple)) and len(s) == 2 and isinstance(s[0], list) and len(s[0]) > 0
                    and all(is_id(t) and t > 0 for t in s[0]) and isinstance(s[1], float))
    if any(not ok(s) for s in sb):
        raise ValueError(f"Each element in `sequence_bias` has to be a non-empty list of lists of positive integers and float, but is {sb}.")
    return {tuple(s[0]): s[1] for s in sb}


def _resolve_row_processors(V: int, eos: int, sequence_bias=None, bad_words_ids=None, min_length=None, forced_eos_token_id=None,
                            exponential_decay_length_penalty=None, begin_suppress_tokens=None):
    """One request's remaining HF logits processors as the engine takes them: (records [(kind, ids, bias)], flags, decay_start,
    decay_factor, min_length).  Gating is transformers' `_get_logits_processor` (None is off; `min_length` acts for > 0); values HF's
    constructors refuse raise with HF's wording, a token id >= V as its first call does.  A single-token bad word equal to `eos` is
    dropped, as HF drops it.  Only the call's own eos can be forced."""
    import numbers
    is_id = lambda t: isinstance(t, numbers.Integral) and not isinstance(t, bool)
    records = []

    def in_vocab(seqs):
        bad = [int(t) for ids in seqs for t in ids if t >= V]
        if bad:
            raise ValueError(f"The model vocabulary size is {V}, but the following tokens were being biased: {bad}")

    if sequence_bias is not None:
        sb = _sequence_bias_dict(sequence_bias)
        in_vocab(sb)
        records += [(_lib.PROC_KIND_BIAS, [int(t) for t in ids], float(b)) for ids, b in sb.items()]
    if bad_words_ids is not None:
        bw = bad_words_ids
        if not isinstance(bw, list) or len(bw) == 0:
            raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bw}.")
        if any(not isinstance(ids, list) for ids in bw):
            raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bw}.")
        if any(any((not is_id(t) or t < 0) for t in ids) for ids in bw):
            raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bw}.")
        banned = _sequence_bias_dict({tuple(ids): float("-inf") for ids in bw if list(ids) != [eos]})
        in_vocab(banned)
        records += [(_lib.PROC_KIND_BAN, [int(t) for t in ids], 0.0) for ids in banned]
    floor = 0
    if min_length is not None:
        if not is_id(min_length) or min_length < 0:
            raise ValueError(f"`min_length` has to be a non-negative integer, but is {min_length}")
        floor = int(min_length)
    flags, start, factor = 0, 0, 0.0
    if forced_eos_token_id is not None:
        if not is_id(forced_eos_token_id) or int(forced_eos_token_id) != int(eos):
            raise ValueError(f"`forced_eos_token_id` can only force the call's own eos_token_id ({eos}), one id per request (a list is "
                             f"read as one value per request, not as HF's list of ids), but is {forced_eos_token_id}")
        flags |= _lib.PROC_FORCED_EOS
    if exponential_decay_length_penalty is not None:
        d = exponential_decay_length_penalty
        if not (isinstance(d, (list, tuple)) and len(d) == 2 and is_id(d[0]) and isinstance(d[1], numbers.Real) and float(d[1]) > 0.0
                and float(d[1]) != float("inf")):
            raise ValueError(f"`exponential_decay_length_penalty` has to be a (start_index, decay_factor) pair of an integer and a "
                             f"positive float, but is {d}")
        flags |= _lib.PROC_DECAY
        start, factor = int(d[0]), float(d[1])
    if begin_suppress_tokens is not None and len(begin_suppress_tokens) > 0:
        ids = list(begin_suppress_tokens)
        if any(not is_id(t) or t < 0 or t >= V for t in ids):
            raise ValueError(f"`begin_suppress_tokens` has to be a list of token ids in [0, {V}), but is {ids}")
        records.append((_lib.PROC_KIND_BEGIN, [int(t) for t in ids], 0.0))
    return records, flags, start, factor, floor


def _proc_table(B: int, V: int, eos: int, **kw):
    """The processor table of a call (`_lib.RowProcessorsC` x B) from the `_PROC_ARGS` (`_split_row_processors` says which values are
    per request), or None when no request has a device control on; and every request's `min_length`.  A request beyond the table's
    capacity per row raises ValueError, as the engine would refuse it (QTTS_ERR_LIMIT)."""
    cols = _split_row_processors(B, **kw)
    if not cols:
        return None, [0] * B
    rows = (_lib.RowProcessorsC * B)()
    on, floors = False, []
    for b in range(B):
        records, flags, start, factor, floor = _resolve_row_processors(V, eos, **{k: v[b] for k, v in cols.items()})
        floors.append(floor)
        n_tok = sum(len(ids) for _, ids, _ in records)
        if len(records) > _lib.PROC_MAX_RECORDS or n_tok > _lib.PROC_MAX_TOKENS:
            raise ValueError(f"request {b}: {len(records)} sequences with {n_tok} tokens exceed the engine's capacity per request "
                             f"({_lib.PROC_MAX_RECORDS} sequences, {_lib.PROC_MAX_TOKENS} tokens)")
        words = []
        for kind, ids, bias in records:
            words += [kind, len(ids), C.c_int32.from_buffer_copy(C.c_float(bias)).value] + ids
        e = rows[b]
        e.decay_factor, e.decay_start, e.flags, e.n_records, e.n_words = factor, start, flags, len(records), len(words)
        e.records[:len(words)] = words
        on = on or bool(flags or records)
    return (rows if on else None), floors


def _is_row_seq(v) -> bool:
    """A per-request value list (list / tuple / 1-d array or tensor) as opposed to one value for the whole batch."""
    if isinstance(v, (list, tuple)):
        return True
    return hasattr(v, "ndim") and hasattr(v, "__len__") and v.ndim == 1


def _scalar(v):
    return v.item() if hasattr(v, "item") and getattr(v, "ndim", 1) == 0 else v


class TalkerEngine:
    """Owns one `qtts_talker` handle."""

    def __init__(self, config: Any, state_dict: Dict[str, torch.Tensor], weight_dtype: torch.dtype = torch.bfloat16,
                 device: str = "cuda:0", max_batch: int = 8, max_seq: int = 4096, use_graph: bool = True, shared_device: bool = False,
                 kv_pages: Optional[int] = None, weight_format: Optional[str] = None):
        """`weight_format`: None (the engine as it is) or "fp8": the talker layers' decode operators as e4m3 codes with a power-of-two scale
        per output row -- half the bytes per frame for them (bf16 engines only; include/qtts.h `qtts_talker_set_weight_format`).  The engine
        is then, bit for bit, the bf16 engine of `fp8.effective_state_dict(config, state_dict)`; `packed_weight_bytes` says what it holds.

        `kv_pages`: the talker's KV cache as a shared pool of that many 16-key pages (`kv_page_bytes` each) instead of `max_batch` x
        `max_seq` keys reserved per row (include/qtts.h `qtts_talker_set_kv_pool`); at least ceil(max_seq / 16).  A continuous stream then
        takes pages as its rows grow and `generate(schedule="continuous")` preempts by restart when the pool runs dry (`_refill_stream`);
        every other call reserves its worst case when it begins.  None: the static layout.

        `shared_device`: this engine will run BESIDE another talker engine on the same device (a throughput job with several engines per GPU:
        bench.py --workload clone-shard, `sharding.engine_partition`).  It then keeps the decode GEMMs where an engine that has the device to
        itself runs the code predictor's MLP as one launch at batch 9..32 (csrc/cp_mlp32.hip): that launch's workgroups wait for each other, and
        behind another engine's kernels they are placed one by one and spin meanwhile -- measured on the MI355X, two engines x waves of 32:
        86.6 k tokens/s with it against 125-127 k without (profiles/r06_cp_mlp32.md); alone on the device it is 6 % faster per frame."""
        self.config = TalkerConfig.from_any(config)
        self.device = _lib.hip_device(device, "TalkerEngine")
        self.weight_dtype = weight_dtype
        self.max_batch, self.max_seq = int(max_batch), int(max_seq)
        self.kv_pages = int(kv_pages) if kv_pages else None
        if weight_format not in (None, "fp8"):
            raise ValueError(f"weight_format must be None or 'fp8', not {weight_format!r}")
        if weight_format == "fp8" and weight_dtype != torch.bfloat16:
            raise ValueError("weight_format='fp8' needs a bf16 engine (weight_dtype=torch.bfloat16); the fp32 engine is the exact parity mode")
        self.weight_format = weight_format
        self._lib = _lib.load_library()
        self._lock = threading.RLock()
        c = self.config
        tc = _lib.TalkerConfigC()
        for f in ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
                  "num_key_value_heads", "head_dim", "num_code_groups", "text_hidden_size", "codec_eos_token_id",
                  "cp_vocab_size", "cp_hidden_size", "cp_intermediate_size", "cp_num_hidden_layers",
                  "cp_num_attention_heads", "cp_num_key_value_heads", "cp_head_dim"):
            setattr(tc, f, int(getattr(c, f)))
        tc.rms_norm_eps, tc.rope_theta = float(c.rms_norm_eps), float(c.rope_theta)
        tc.cp_rms_norm_eps, tc.cp_rope_theta = float(c.cp_rms_norm_eps), float(c.cp_rope_theta)
        tc.weight_dtype = _lib.QTTS_BF16 if weight_dtype == torch.bfloat16 else _lib.QTTS_F32
        tc.max_batch, tc.max_seq, tc.use_graph = self.max_batch, self.max_seq, 1 if use_graph else 0
        self._h = C.c_void_p()
        import contextlib
        with torch.cuda.device(self.device), (_lib.options(QTTS_CP_MLP32="0") if shared_device else contextlib.nullcontext()):
            _lib.check(self._lib.qtts_talker_create(C.byref(tc), C.byref(self._h)))
            if self.kv_pages:
                _lib.check(self._lib.qtts_talker_set_kv_pool(self._h, self.kv_pages))
            if self.weight_format == "fp8":
                _lib.check(self._lib.qtts_talker_set_weight_format(self._h, _lib.WEIGHTS_FP8))
            has_prefix = any(k.startswith("talker.") for k in state_dict)
            for name, t in state_dict.items():
                if has_prefix:
                    if not name.startswith("talker."):
                        continue
                    name = name[len("talker."):]
                if name.startswith(_SKIP_PREFIXES):
                    continue
                _lib.bind_tensor(self._lib.qtts_talker_bind, self._h, name, t)
            _lib.bind_tensor(self._lib.qtts_talker_bind, self._h, "model.rotary_emb.inv_freq",
                             _default_inv_freq(c.rope_theta, c.head_dim))
            _lib.bind_tensor(self._lib.qtts_talker_bind, self._h, "code_predictor.model.rotary_emb.inv_freq",
                             _default_inv_freq(c.cp_rope_theta, c.cp_head_dim))
            _lib.check(self._lib.qtts_talker_finalize(self._h))
            # hipGraph capture needs a non-default stream; everything the engine does runs on this one
            self._stream = torch.cuda.Stream(device=self.device)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.qtts_talker_destroy(h)

    def _s(self):
        return C.c_void_p(self._stream.cuda_stream)

    @property
    def kv_page_bytes(self) -> int:
        """Bytes of one 16-key page of the talker cache over all layers, K and V: layers x 2 x kv heads x 16 x head_dim x element size
        (1.7B dims in bf16: 28 x 2 x 8 x 16 x 128 x 2 B = 1.835 MB)."""
        c = self.config
        return int(c.num_hidden_layers) * 2 * int(c.num_key_value_heads) * 16 * int(c.head_dim) * (2 if self.weight_dtype == torch.bfloat16 else 4)

    @property
    def packed_weight_bytes(self) -> int:
        """Bytes of every packed decode operator the engine holds on the device (an fp8 operator: N K + 4 N; its bf16 form: 2 N K)."""
        n = C.c_int64(0)
        _lib.check(self._lib.qtts_talker_weight_format(self._h, None, C.byref(n)))
        return int(n.value)

    @_lib.locked
    def set_profile(self, enable):
        """0 / False: off.  1 / True: time every decode-GEMM launch of the real frame step on its own (see `gemm_profile`).
        2: round 2's measurement, the GEMM launches of one frame step replayed in isolation (that call yields no codes)."""
        _lib.check(self._lib.qtts_talker_set_profile(self._h, int(enable)))

    @_lib.locked
    def gemm_profile(self) -> List[dict]:
        """Per-class result of the last generate call made under `set_profile(1)` (include/qtts.h `qtts_gemm_class`)."""
        buf = (_lib.GemmClassC * 64)()
        n = C.c_int32(0)
        _lib.check(self._lib.qtts_talker_get_gemm_profile(self._h, buf, 64, C.byref(n)))
        return [{f[0]: getattr(buf[i], f[0]) for f in buf[i]._fields_} for i in range(min(64, n.value))]

    @_lib.locked
    def stats(self) -> dict:
        st = _lib.TalkerStatsC()
        _lib.check(self._lib.qtts_talker_get_stats(self._h, C.byref(st)))
        out = {f[0]: getattr(st, f[0]) for f in st._fields_}
        # (`qtts_talker_stats` keeps its layout under ABI 15: the per-row-position mode's two figures come from a call of their own)
        rp, longest = C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.qtts_talker_stream_mode(self._h, C.byref(rp), C.byref(longest)))
        out["row_positions"], out["max_row_len"] = int(rp.value), int(longest.value)
        return out

    # ------------------------------------------------------------------ text_projection (prompt assembly)
    @_lib.locked
    def text_projection(self, x: torch.Tensor) -> torch.Tensor:
        """Qwen3TTSTalkerResizeMLP (M:808-816): (..., text_hidden) -> (..., hidden), fp32."""
        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).to(self.device, torch.float32).contiguous()
        y = torch.empty(x2.shape[0], self.config.hidden_size, dtype=torch.float32, device=self.device)
        cur = torch.cuda.current_stream(self.device)
        self._stream.wait_stream(cur)
        with torch.cuda.device(self.device), torch.cuda.stream(self._stream):
            _lib.check(self._lib.qtts_talker_text_projection(self._h, C.c_void_p(x2.data_ptr()), x2.shape[0],
                                                             C.c_void_p(y.data_ptr()), self._s()))
        cur.wait_stream(self._stream)
        x2.record_stream(self._stream)
        return y.reshape(*shp[:-1], self.config.hidden_size)

    def _clamp_new_tokens(self, T: int, max_new_tokens: int) -> int:
        """HF treats `max_new_tokens` as an upper bound (generation_config.json of the released checkpoints asks for 8192);
        the engine's KV capacity is `max_seq`, fixed at construction.  A request that asks for more than fits is cut at the
        capacity (with a warning, once) instead of being refused; a prompt that leaves no room at all is an error."""
        room = self.max_seq - T
        if room < 1:
            raise ValueError(f"prompt ({T} rows) does not fit max_seq ({self.max_seq}) given at construction")
        if max_new_tokens > room:
            if not getattr(self, "_warned_clamp", False):
                import warnings
                warnings.warn(f"max_new_tokens={max_new_tokens} exceeds the KV capacity left after the prompt "
                              f"(max_seq {self.max_seq} - prompt {T} = {room}); generation is capped at {room} tokens. "
                              f"Pass a larger max_seq at construction for longer utterances.")
                self._warned_clamp = True
            max_new_tokens = room
        return max_new_tokens

    def _row_table(self, B: int, T, force: bool = False, **kw):
        """The per-request settings table of a call (include/qtts.h `qtts_row_sampling`), or None when every argument of `_ROW_ARGS`
        is a scalar (the scalar path).  Any of them may be a sequence of length B; scalars are broadcast.  Every element goes through
        the checks a scalar goes through (`_check_warpers`, `_resolve_top`, `_clamp_new_tokens`).  Seeds: a `None` (the whole argument
        or one element) draws a fresh seed for each such row; ONE integer s gives request b the seed s + b, so that requests never share
        their draws unless a seed list says so.  `T`: the prompt length the limits are clamped against, one for the batch or a list of
        B (the refill schedules: every request against its own prompt).  `force`: the table is built whatever the arguments are (a call
        with a warper table, `_warp_table`, which lives on the per-row table; the refill schedules): scalars are broadcast.  Returns
        (ctypes array of B entries, the largest max_new_tokens)."""
        if not force and not any(_is_row_seq(kw[k]) for k in _ROW_ARGS):
            return None
        cols = {}
        for k in _ROW_ARGS:
            v = kw[k]
            if _is_row_seq(v):
                v = [_scalar(x) for x in v]
                if len(v) != B:
                    raise ValueError(f"`{k}` has {len(v)} entries for a batch of {B} requests")
            elif k == "seed" and v is not None:
                # the table's Philox counter has no row term: ONE seed for every row would give every request the same random numbers
                v = [int(v) + b for b in range(B)]
            else:
                v = [v] * B
            cols[k] = v
        rows = (_lib.RowSamplingC * B)()
        for b in range(B):
            r = {k: cols[k][b] for k in _ROW_ARGS}
            e = rows[b]
            _fill_sampling(e, r)
            if r["max_new_tokens"] is None or int(r["max_new_tokens"]) < 1:
                raise ValueError(f"`max_new_tokens` of request {b} must be a positive integer, but is {r['max_new_tokens']}")
            e.max_new_tokens = self._clamp_new_tokens(T[b] if isinstance(T, list) else T, int(r["max_new_tokens"]))
            e.min_new_tokens = int(r["min_new_tokens"]) if r["min_new_tokens"] is not None else 0
        return rows, max(int(rows[b].max_new_tokens) for b in range(B))

    # ------------------------------------------------------------------ generate (seam S2)
    @_lib.locked
    def text_embed(self, ids: torch.Tensor) -> torch.Tensor:
        """text_projection(text_embedding[ids]) on device (M:2076-2080): ids int64 (n,) -> (n, H) fp32."""
        ids = ids.reshape(-1).to(self.device, torch.long).contiguous()
        y = torch.empty(ids.numel(), self.config.hidden_size, dtype=torch.float32, device=self.device)
        if ids.numel() == 0:
            return y
        self._stream.wait_stream(torch.cuda.current_stream(self.device))     # `ids` was produced on the caller's stream
        with torch.cuda.device(self.device), torch.cuda.stream(self._stream):
            _lib.check(self._lib.qtts_talker_text_embed(self._h, C.c_void_p(ids.data_ptr()), ids.numel(),
                                                        C.c_void_p(y.data_ptr()), self._s()))
        torch.cuda.current_stream(self.device).wait_stream(self._stream)
        return y

    @_lib.locked
    def assemble_rows(self, desc: torch.Tensor, proj: Optional[torch.Tensor] = None, spk: Optional[torch.Tensor] = None,
                      ref_codes: Optional[torch.Tensor] = None) -> torch.Tensor:
        """out[r] = proj[text_row] + codec-side term, from int32 descriptors (rows, 4) = {text_row, codec_id, spk_row,
        ref_frame} (-1 = absent).  See include/qtts.h `qtts_talker_assemble_rows`."""
        dev = self.device
        desc = desc.reshape(-1, 4).to(dev, torch.int32).contiguous()
        out = torch.empty(desc.shape[0], self.config.hidden_size, dtype=torch.float32, device=dev)
        if desc.shape[0] == 0:
            return out
        proj = None if proj is None or proj.numel() == 0 else proj.to(dev, torch.float32).contiguous()
        spk = None if spk is None or spk.numel() == 0 else spk.to(dev, torch.float32).contiguous()
        ref = None if ref_codes is None or ref_codes.numel() == 0 else ref_codes.to(dev, torch.long).contiguous()
        if ref is not None and (ref.dim() != 2 or ref.shape[1] != self.config.num_code_groups):
            raise ValueError(f"ref_codes must be (frames, {self.config.num_code_groups})")
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
        self._stream.wait_stream(torch.cuda.current_stream(dev))             # desc / proj / spk / ref come from the caller's stream
        with torch.cuda.device(dev), torch.cuda.stream(self._stream):
            _lib.check(self._lib.qtts_talker_assemble_rows(
                self._h, C.c_void_p(desc.data_ptr()), desc.shape[0], ptr(proj), 0 if proj is None else proj.shape[0],
                ptr(spk), 0 if spk is None else spk.shape[0], ptr(ref), 0 if ref is None else ref.shape[0],
                C.c_void_p(out.data_ptr()), self._s()))
        torch.cuda.current_stream(dev).wait_stream(self._stream)
        return out

    @_lib.locked
    def generate(self, *args, **kw) -> TalkerGenerateOutput:
        """Seam S2 (`talker.generate`, M:2272): see `_prepare` and `_generate_once` for the arguments.  One thing is added around it: a generation
        that ended on the fused launches' give-up flag (a consumer workgroup lost its producers -- another PROCESS on the device took
        the compute units; csrc/talker_engine.hip: check_fused_flag) has produced nothing the caller saw, and the engine has left the
        fused launches for good, so the request is re-run ONCE here on the separate launches instead of surfacing a bare error.
        (`generate_stream` cannot do that after it has yielded packets: there the error reaches the caller, whose retry runs on the
        separate launches.)"""
        schedule = kw.pop("schedule", "waves")
        if schedule in ("refill", "continuous"):
            return self._generate_refill(*args, row_positions=schedule == "continuous", **kw)
        if schedule != "waves":
            raise ValueError(f"`schedule` must be 'waves', 'refill' or 'continuous', but is {schedule!r}")
        giveups = self.stats()["cp_fused_giveups"]
        try:
            return self._generate_once(*args, **kw)
        except _lib.QttsError:
            if self.stats()["cp_fused_giveups"] <= giveups:
                raise
            import warnings
            warnings.warn("a fused code-predictor launch gave up waiting for its producers (device shared with another process?); "
                          "this engine now runs the separate launches and the request is re-run once")
            return self._generate_once(*args, **kw)

    def _prepare(self, queue_mode: bool, inputs_embeds: torch.Tensor, attention_mask: torch.Tensor, trailing_text_hidden: torch.Tensor,
                 tts_pad_embed: torch.Tensor, max_new_tokens: int = 2048, min_new_tokens: int = 2,
                 do_sample: bool = True, top_k: Optional[int] = 50, top_p: Optional[float] = 1.0,
                 temperature: Optional[float] = 0.9, subtalker_dosample: bool = True,
                 subtalker_top_k: Optional[int] = 50, subtalker_top_p: Optional[float] = 1.0,
                 subtalker_temperature: Optional[float] = 0.9, eos_token_id: Optional[int] = None,
                 repetition_penalty: float = 1.05, suppress_tokens: Optional[List[int]] = None, seed: Optional[int] = None,
                 min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None, no_repeat_ngram_size=None,
                 sequence_bias=None, bad_words_ids=None, min_length=None, forced_eos_token_id=None,
                 exponential_decay_length_penalty=None, begin_suppress_tokens=None, **unused) -> _Call:
        """The arguments of a generation call (`generate`, `generate_stream` and the refill schedules take them alike), checked and
        made ready: shapes, the left-padded mask, the per-row and warper tables or the scalar settings, eos and the suppress list, the
        three tensors on the device.  `queue_mode` (the refill schedules): the rows are a queue of requests, not a batch -- any number
        of them, always on the per-row table, every request's limit clamped against the room its OWN prompt leaves.

        Per-request settings: each of `do_sample`, `top_k`, `top_p`, `temperature`, `repetition_penalty`, the four `subtalker_*`
        knobs, `max_new_tokens`, `min_new_tokens` and `seed` is one value for the batch (as in the reference) or a sequence of B
        values, one per request.  With any sequence the call runs on the engine's per-row table (`qtts_talker_generate_rows`): a
        request's draws then depend on its own seed only -- not on its row or on the other requests -- and changing the values between
        calls does not re-capture the frame graph.  Request b's frames are `codes[b]` up to its first eos in codebook 0; a request
        that reached its own `max_new_tokens` m receives eos from `tokens[b, m - 1]` on (a scalar run keeps the sampled token there).

        `min_p`, `typical_p`, `epsilon_cutoff`, `eta_cutoff` and `no_repeat_ngram_size` (HF generate's remaining sampling controls, for
        the codebook-0 sampler; gating and errors as in transformers, `_resolve_row_warpers`) are one value or a sequence of B as well.
        Any of them that is on puts the call on the per-row table (scalars are broadcast; ONE integer seed s gives request b the seed
        s + b) and the talker's sampler becomes `sample_warp_kernel` (`sampler_class()` reports 3).

        `sequence_bias`, `bad_words_ids`, `min_length`, `forced_eos_token_id`, `exponential_decay_length_penalty` and
        `begin_suppress_tokens` (HF generate's remaining logits processors, for the codebook-0 sampler; chain order, gating and errors
        as in transformers: `_resolve_row_processors`, include/qtts.h `qtts_row_processors`) each take HF's own form of the value for
        the whole call or a list with one such value -- or None, off -- per request (`_split_row_processors`).  A request's `cur_len`
        is its own generated count, under every schedule.  `min_length` is folded into the request's EOS floor,
        max(min_length, min_new_tokens), and needs no device work; any of the others that is on puts the call on the per-row table
        and on `sample_warp_kernel` like a warper.  `forced_eos_token_id` can only be the call's own eos: at the request's token index
        limit - 1 every score but EOS is removed, where limit is the request's EFFECTIVE `max_new_tokens` -- after the clamp to the
        room `max_seq` leaves (`_clamp_new_tokens`); it comes behind the EOS floor in the chain and wins over it.
        `exponential_decay_length_penalty=(start, factor)`: the power factor ** (cur_len - start) is evaluated in double on the
        device, the rest in fp32, as HF does.  Any OTHER keyword this signature does not name is still swallowed."""
        c, dev = self.config, self.device
        if inputs_embeds.dim() != 3 or inputs_embeds.shape[-1] != c.hidden_size:
            raise ValueError(f"inputs_embeds must be (B, T, {c.hidden_size})")
        B, T, H = inputs_embeds.shape
        if not queue_mode:
            if B > self.max_batch:
                raise ValueError(f"batch {B} exceeds max_batch {self.max_batch} given at construction")
            self._live_batch = int(B)
        mask = attention_mask.to("cpu", torch.long)
        if mask.shape != (B, T):
            raise ValueError("attention_mask must be (B, T)")
        n_pad = (1 - mask).sum(-1)
        # the reference only ever builds LEFT-padded masks (M:2251-2254); anything else is not this path
        expect = (torch.arange(T)[None, :] >= n_pad[:, None]).long()
        if not torch.equal(mask, expect) or int(n_pad.max()) >= T:
            raise ValueError("attention_mask must be left-padded: [0]*n_pad + [1]*(T-n_pad) per row")
        n_pad = [int(x) for x in n_pad]
        lens = [T - x for x in n_pad]
        # (a request keeps its entries of both tables through queueing, admission and restart)
        warp = _warp_table(B, min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff,
                           no_repeat_ngram_size=no_repeat_ngram_size)
        eos = c.codec_eos_token_id if eos_token_id is None else int(eos_token_id)
        proc, floors = _proc_table(B, c.vocab_size, eos, sequence_bias=sequence_bias, bad_words_ids=bad_words_ids, min_length=min_length,
                                   forced_eos_token_id=forced_eos_token_id,
                                   exponential_decay_length_penalty=exponential_decay_length_penalty,
                                   begin_suppress_tokens=begin_suppress_tokens)
        if any(floors):          # MinLength and MinNewTokensLength block the same token: one floor per request
            mins = [_scalar(x) for x in min_new_tokens] if _is_row_seq(min_new_tokens) else [min_new_tokens] * B
            if len(mins) != B:
                raise ValueError(f"`min_new_tokens` has {len(mins)} entries for a batch of {B} requests")
            mins = [max(int(m) if m is not None else 0, f) for m, f in zip(mins, floors)]
            min_new_tokens = mins if _is_row_seq(min_new_tokens) or len(set(mins)) > 1 else mins[0]
        knobs = dict(do_sample=do_sample, top_k=top_k, top_p=top_p, temperature=temperature, repetition_penalty=repetition_penalty,
                     subtalker_dosample=subtalker_dosample, subtalker_top_k=subtalker_top_k, subtalker_top_p=subtalker_top_p,
                     subtalker_temperature=subtalker_temperature, max_new_tokens=max_new_tokens, min_new_tokens=min_new_tokens, seed=seed)
        table = self._row_table(B, lens if queue_mode else T, force=queue_mode or warp is not None or proc is not None, **knobs)
        rows = sp = None
        if table is not None:
            rows, max_new_tokens = table                  # buffers are sized by the largest limit
        else:
            max_new_tokens = self._clamp_new_tokens(T, int(max_new_tokens))
            sp = _lib.SamplingC()
            _fill_sampling(sp, knobs)
        suppress = [] if suppress_tokens is None else list(suppress_tokens)
        emb = inputs_embeds.to(dev, torch.float32).contiguous()
        trail = trailing_text_hidden.to(dev, torch.float32).contiguous()
        if trail.dim() != 3 or trail.shape[0] != B or trail.shape[2] != H or trail.shape[1] < 1:
            raise ValueError("trailing_text_hidden must be (B, Tt >= 1, H)")
        pad = tts_pad_embed.to(dev, torch.float32).reshape(-1).contiguous()
        if pad.numel() != H:
            raise ValueError("tts_pad_embed must have H elements")
        return _Call(B=B, T=T, n_pad=n_pad, lens=lens, emb=emb, trail=trail, pad=pad,
                     eos=eos, suppress=suppress,
                     npad_c=(C.c_int32 * B)(*n_pad), sup_c=(C.c_int32 * max(1, len(suppress)))(*[int(x) for x in suppress]),
                     rows=rows, warp=warp, proc=proc, sp=sp, max_new_tokens=max_new_tokens, min_new_tokens=min_new_tokens)

    def _generate_once(self, inputs_embeds: torch.Tensor, *args, output_hidden_states: bool = True,
                       teacher_codes: Optional[torch.Tensor] = None, logit_steps: Optional[List[int]] = None, **kw) -> TalkerGenerateOutput:
        """One static batch (`generate`, the "waves" schedule); the arguments are `_prepare`'s.  `teacher_codes` (B, F, G) switches on
        the diagnostic teacher-forced mode (include/qtts.h `qtts_talker_set_teacher`): greedy, exactly F frames; the engine's own
        choices come back in `.own`, the raw cb-0 logits of the token steps listed in `logit_steps` in `.logits_trace`."""
        c, dev = self.config, self.device
        if teacher_codes is not None:
            if teacher_codes.dim() != 3 or teacher_codes.shape[0] != inputs_embeds.shape[0] or teacher_codes.shape[2] != c.num_code_groups:
                raise ValueError(f"teacher_codes must be (B, F, {c.num_code_groups})")
            F_t = int(teacher_codes.shape[1])
            kw.update(max_new_tokens=F_t + 1, min_new_tokens=F_t + 1, do_sample=False, subtalker_dosample=False)
        p = self._prepare(False, inputs_embeds, *args, **kw)
        if teacher_codes is not None and p.rows is not None:
            raise ValueError("teacher_codes takes scalar settings, not per-request sequences")
        B, T, H, max_new_tokens = p.B, p.T, c.hidden_size, p.max_new_tokens
        emb, trail, pad, suppress_tokens = p.emb, p.trail, p.pad, p.suppress
        max_frames = max(1, max_new_tokens - 1)
        codes = torch.zeros(B, max_frames, c.num_code_groups, dtype=torch.int64, device=dev)
        hidden = torch.zeros(B, max_frames, H, dtype=torch.float32, device=dev) if output_hidden_states else None
        tokens = torch.full((B, max_new_tokens), -1, dtype=torch.int64, device=dev)
        n_frames = C.c_int32(0)
        own = trace = None
        if teacher_codes is not None:
            if F_t != max_new_tokens - 1:
                raise ValueError("teacher_codes: the forced frames do not fit max_seq")
            tc = teacher_codes.to(dev, torch.long).contiguous()
            # forced codes index embedding tables on the device: range-check them here (cb-0 < vocab, sub-codes < cp vocab)
            if int(tc.min()) < 0 or int(tc[..., 0].max()) >= c.vocab_size or (tc.shape[2] > 1 and int(tc[..., 1:].max()) >= c.cp_vocab_size):
                raise ValueError("teacher_codes: code index out of range")
            own = torch.full((B, F_t + 1, c.num_code_groups), -1, dtype=torch.int32, device=dev)
            slots = trace = None
            if logit_steps:
                sl = [-1] * (F_t + 1)
                for k, i in enumerate(logit_steps):
                    if not 0 <= int(i) <= F_t:
                        raise ValueError("logit_steps entries must be token steps in [0, F]")
                    sl[int(i)] = k
                slots = torch.tensor(sl, dtype=torch.int32, device=dev)
                trace = torch.zeros(len(logit_steps), B, c.vocab_size, dtype=torch.float32, device=dev)
        cur = torch.cuda.current_stream(dev)
        self._stream.wait_stream(cur)
        with torch.cuda.device(dev), torch.cuda.stream(self._stream):
            _lib.check(self._lib.qtts_talker_prefill(self._h, C.c_void_p(emb.data_ptr()), B, T, p.npad_c,
                                                     C.c_void_p(trail.data_ptr()), trail.shape[1],
                                                     C.c_void_p(pad.data_ptr()), self._s()))
            if teacher_codes is not None:
                _lib.check(self._lib.qtts_talker_set_teacher(self._h, C.c_void_p(tc.data_ptr()), F_t, C.c_void_p(own.data_ptr()),
                                                             C.c_void_p(slots.data_ptr()) if trace is not None else None,
                                                             C.c_void_p(trace.data_ptr()) if trace is not None else None))
            out_c = (C.c_void_p(codes.data_ptr()), C.c_void_p(hidden.data_ptr()) if hidden is not None else None,
                     C.c_void_p(tokens.data_ptr()), C.byref(n_frames), self._s())
            try:
                if p.rows is not None:
                    if p.warp is not None:
                        _lib.check(self._lib.qtts_talker_set_row_warpers(self._h, p.warp, B))
                    if p.proc is not None:
                        _lib.check(self._lib.qtts_talker_set_row_processors(self._h, p.proc, B))
                    _lib.check(self._lib.qtts_talker_generate_rows(self._h, p.rows, B, p.eos, p.sup_c, len(suppress_tokens), *out_c))
                else:
                    _lib.check(self._lib.qtts_talker_generate(self._h, C.byref(p.sp), int(max_new_tokens), int(p.min_new_tokens), p.eos,
                                                              p.sup_c, len(suppress_tokens), *out_c))
            finally:
                if teacher_codes is not None:
                    _lib.check(self._lib.qtts_talker_set_teacher(self._h, None, 0, None, None, None))
        cur.wait_stream(self._stream)
        nf = int(n_frames.value)
        return TalkerGenerateOutput(codes=codes[:, :nf], hidden=hidden[:, :nf] if hidden is not None else None,
                                    tokens=tokens[:, : nf + 1], n_frames=nf, own=own, logits_trace=trace)

    def generate_stream(self, inputs_embeds: torch.Tensor, attention_mask: torch.Tensor, trailing_text_hidden: torch.Tensor,
                        tts_pad_embed: torch.Tensor, packet_frames: int = 4, max_new_tokens: int = 2048, min_new_tokens: int = 2,
                        do_sample: bool = True, top_k: Optional[int] = 50, top_p: Optional[float] = 1.0,
                        temperature: Optional[float] = 0.9, subtalker_dosample: bool = True,
                        subtalker_top_k: Optional[int] = 50, subtalker_top_p: Optional[float] = 1.0,
                        subtalker_temperature: Optional[float] = 0.9, eos_token_id: Optional[int] = None,
                        repetition_penalty: float = 1.05, suppress_tokens: Optional[List[int]] = None,
                        seed: Optional[int] = None, schedule: str = "waves", min_p=None, typical_p=None, epsilon_cutoff=None,
                        eta_cutoff=None, no_repeat_ngram_size=None, sequence_bias=None, bad_words_ids=None, min_length=None,
                        forced_eos_token_id=None, exponential_decay_length_penalty=None, begin_suppress_tokens=None, **unused):
        """Streaming OUTPUT (include/qtts.h `qtts_talker_stream_*`): a generator that yields `codes[:, f0:f1]` (B, k, G)
        int64 device tensors, k <= packet_frames, as the frames are produced; same arguments (per-request sequences included) and the
        same frames as `generate`.  Closing the generator early abandons the request.  Holds the engine lock while active.

        `schedule="refill"`: any number of requests on `max_batch` rows, scheduled as `generate(schedule="refill")` schedules them (same
        admission rule, per-row table and seed rules: `_refill_stream`); yields one `RefillPacket` per packet of the running stream
        instead of a block of codes.  Concatenating a request's packets gives exactly the codes `generate(schedule="refill")` returns
        for it.  `schedule="continuous"`: the same on ONE stream with per-row positions (`_refill_stream(row_positions=True)`)."""
        kw = dict(max_new_tokens=max_new_tokens, min_new_tokens=min_new_tokens, do_sample=do_sample, top_k=top_k, top_p=top_p,
                  temperature=temperature, subtalker_dosample=subtalker_dosample, subtalker_top_k=subtalker_top_k,
                  subtalker_top_p=subtalker_top_p, subtalker_temperature=subtalker_temperature, eos_token_id=eos_token_id,
                  repetition_penalty=repetition_penalty, suppress_tokens=suppress_tokens, seed=seed, min_p=min_p, typical_p=typical_p,
                  epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff, no_repeat_ngram_size=no_repeat_ngram_size,
                  sequence_bias=sequence_bias, bad_words_ids=bad_words_ids, min_length=min_length, forced_eos_token_id=forced_eos_token_id,
                  exponential_decay_length_penalty=exponential_decay_length_penalty, begin_suppress_tokens=begin_suppress_tokens)
        if schedule in ("refill", "continuous"):
            yield from self._refill_stream(inputs_embeds, attention_mask, trailing_text_hidden, tts_pad_embed, packet_frames=packet_frames,
                                           row_positions=schedule == "continuous", **kw)
            return
        if schedule != "waves":
            raise ValueError(f"`schedule` must be 'waves', 'refill' or 'continuous', but is {schedule!r}")
        if packet_frames < 1:
            raise ValueError("packet_frames must be >= 1")
        p = self._prepare(False, inputs_embeds, attention_mask, trailing_text_hidden, tts_pad_embed, **kw)
        dev, B, n_sup = self.device, p.B, len(p.suppress)
        codes = torch.zeros(B, max(1, p.max_new_tokens - 1), self.config.num_code_groups, dtype=torch.int64, device=dev)
        total, fin, nf = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        with self._lock:
            self._stream.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.device(dev), torch.cuda.stream(self._stream):
                _lib.check(self._lib.qtts_talker_prefill(self._h, C.c_void_p(p.emb.data_ptr()), B, p.T, p.npad_c,
                                                         C.c_void_p(p.trail.data_ptr()), p.trail.shape[1],
                                                         C.c_void_p(p.pad.data_ptr()), self._s()))
                if p.rows is not None:
                    if p.warp is not None:
                        _lib.check(self._lib.qtts_talker_set_row_warpers(self._h, p.warp, B))
                    if p.proc is not None:
                        _lib.check(self._lib.qtts_talker_set_row_processors(self._h, p.proc, B))
                    _lib.check(self._lib.qtts_talker_stream_begin_rows(self._h, p.rows, B, p.eos, p.sup_c, n_sup,
                                                                       C.c_void_p(codes.data_ptr()), None, self._s()))
                else:
                    _lib.check(self._lib.qtts_talker_stream_begin(self._h, C.byref(p.sp), int(p.max_new_tokens), int(p.min_new_tokens),
                                                                  p.eos, p.sup_c, n_sup, C.c_void_p(codes.data_ptr()), None, self._s()))
            seen = 0
            try:
                while not fin.value:
                    with torch.cuda.device(dev), torch.cuda.stream(self._stream):
                        _lib.check(self._lib.qtts_talker_stream_step(self._h, int(packet_frames), C.byref(total), C.byref(fin),
                                                                     self._s()))
                    if total.value > seen:              # stream_step synchronises: these frames are final
                        yield codes[:, seen:total.value]
                        seen = total.value
            finally:
                with torch.cuda.device(dev), torch.cuda.stream(self._stream):
                    _lib.check(self._lib.qtts_talker_stream_end(self._h, None, C.byref(nf), self._s()))
                torch.cuda.current_stream(dev).wait_stream(self._stream)

    # ------------------------------------------------------------------ admission into finished rows (include/qtts.h, ABI v15)
    @_lib.locked
    def stream_open(self, inputs_embeds: torch.Tensor, n_pad: List[int], trailing_text_hidden: torch.Tensor, tts_pad_embed: torch.Tensor,
                    rows, max_row_tokens: int, eos_token_id: int, suppress_tokens: List[int], output_hidden_states: bool = False,
                    row_positions: bool = False, warpers=None, processors=None):
        """Prefill + `qtts_talker_stream_begin_admitting`: `rows` is a `_lib.RowSamplingC` array with one entry per row of
        `inputs_embeds` (B, T, H; row b left-padded by n_pad[b]).  Returns (codes (B, max_row_tokens - 1, G), hidden or None): the
        blocks the stream fills, ONE occupant per row at a time -- copy a finished row out before `stream_admit` re-uses it.
        `row_positions=True` opens the stream with `qtts_talker_stream_begin_admitting_rows`: every row carries its own KV length, an
        admitted prompt restarts its row at its own length, and `stream_row_lens()` reads the lengths back.  `warpers`: a
        `_lib.RowWarpersC` array with one entry per row (`qtts_talker_set_row_warpers`), or None; `processors`: a `_lib.RowProcessorsC`
        array likewise (`qtts_talker_set_row_processors`)."""
        c, dev = self.config, self.device
        B, T, H = inputs_embeds.shape
        if B > self.max_batch:
            raise ValueError(f"batch {B} exceeds max_batch {self.max_batch} given at construction")
        self._live_batch = int(B)
        emb = inputs_embeds.to(dev, torch.float32).contiguous()
        trail = trailing_text_hidden.to(dev, torch.float32).contiguous()
        pad = tts_pad_embed.to(dev, torch.float32).reshape(-1).contiguous()
        F = max(1, int(max_row_tokens) - 1)
        codes = torch.zeros(B, F, c.num_code_groups, dtype=torch.int64, device=dev)
        hidden = torch.zeros(B, F, H, dtype=torch.float32, device=dev) if output_hidden_states else None
        npad_c = (C.c_int32 * B)(*[int(x) for x in n_pad])
        sup_c = (C.c_int32 * max(1, len(suppress_tokens)))(*[int(x) for x in suppress_tokens])
        self._stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.device(dev), torch.cuda.stream(self._stream):
            _lib.check(self._lib.qtts_talker_prefill(self._h, C.c_void_p(emb.data_ptr()), B, T, npad_c, C.c_void_p(trail.data_ptr()),
                                                     trail.shape[1], C.c_void_p(pad.data_ptr()), self._s()))
            begin = self._lib.qtts_talker_stream_begin_admitting_rows if row_positions else self._lib.qtts_talker_stream_begin_admitting
            if warpers is not None:
                _lib.check(self._lib.qtts_talker_set_row_warpers(self._h, warpers, B))
            if processors is not None:
                _lib.check(self._lib.qtts_talker_set_row_processors(self._h, processors, B))
            _lib.check(begin(
                self._h, rows, B, int(max_row_tokens), int(eos_token_id), sup_c, len(suppress_tokens), C.c_void_p(codes.data_ptr()),
                C.c_void_p(hidden.data_ptr()) if hidden is not None else None, self._s()))
        self._open = (codes, hidden)          # (the stream writes these blocks until `stream_close`)
        return codes, hidden

    @_lib.locked
    def stream_admit(self, row_ids: List[int], inputs_embeds: torch.Tensor, n_pad: List[int], trailing_text_hidden: torch.Tensor, rows,
                     warpers=None, processors=None):
        """`qtts_talker_stream_admit`: request i of the group (inputs_embeds (n, T', H) left-padded by n_pad[i], trailing (n, Tt', H),
        settings rows[i], warpers[i] of a `_lib.RowWarpersC` array and processors[i] of a `_lib.RowProcessorsC` array if given) takes the finished row row_ids[i] of the open stream."""
        dev = self.device
        n, T, H = inputs_embeds.shape
        emb = inputs_embeds.to(dev, torch.float32).contiguous()
        trail = trailing_text_hidden.to(dev, torch.float32).contiguous()
        ids_c = (C.c_int32 * n)(*[int(x) for x in row_ids])
        npad_c = (C.c_int32 * n)(*[int(x) for x in n_pad])
        self._stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.device(dev), torch.cuda.stream(self._stream):
            if warpers is not None:
                _lib.check(self._lib.qtts_talker_set_row_warpers(self._h, warpers, n))
            if processors is not None:
                _lib.check(self._lib.qtts_talker_set_row_processors(self._h, processors, n))
            _lib.check(self._lib.qtts_talker_stream_admit(self._h, n, ids_c, C.c_void_p(emb.data_ptr()), T, npad_c,
                                                          C.c_void_p(trail.data_ptr()), trail.shape[1], rows, self._s()))

    @_lib.locked
    def stream_rows(self):
        """`qtts_talker_stream_rows`: (unfinished[B], final frames[B] of each row's occupant, the stream's position kv_len)."""
        B = self._live_batch
        uf, fr, kv = (C.c_int32 * B)(), (C.c_int32 * B)(), C.c_int32(0)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.qtts_talker_stream_rows(self._h, uf, fr, C.byref(kv)))
        return list(uf), list(fr), int(kv.value)

    @_lib.locked
    def stream_row_lens(self) -> List[int]:
        """`qtts_talker_stream_row_lens`: every row's KV length on a stream opened with `row_positions=True` (a finished row: the length
        it froze at)."""
        lens = (C.c_int32 * self._live_batch)()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.qtts_talker_stream_row_lens(self._h, lens))
        return list(lens)

    @_lib.locked
    def stream_kv(self):
        """`qtts_talker_stream_kv` on a pooled engine: (pages held by each row of the last prefill's batch, free pages, pool size)."""
        B = getattr(self, "_live_batch", self.max_batch)
        pages, free, pool = (C.c_int32 * B)(), C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.qtts_talker_stream_kv(self._h, pages, C.byref(free), C.byref(pool)))
        return list(pages), int(free.value), int(pool.value)

    @_lib.locked
    def debug_kv_table(self, row: int) -> List[int]:
        """`qtts_talker_debug_kv_table`: the device page table of one row of the talker cache, ceil(max_seq / 16) entries in slot order
        (pooled: an entry without a grant holds `kv_pages`, the sink)."""
        ent = (C.c_int32 * (-(-self.max_seq // 16)))()
        with torch.cuda.device(self.device), torch.cuda.stream(self._stream):
            _lib.check(self._lib.qtts_talker_debug_kv_table(self._h, int(row), ent, self._s()))
        return list(ent)

    @_lib.locked
    def stream_evict(self, row_ids: List[int]):
        """`qtts_talker_stream_evict`: abandon the occupants of the listed rows of the open stream with per-row positions (preemption by
        restart, or cancelling a request); their pages go back to the pool."""
        ids_c = (C.c_int32 * max(1, len(row_ids)))(*[int(x) for x in row_ids])
        with torch.cuda.device(self.device), torch.cuda.stream(self._stream):
            _lib.check(self._lib.qtts_talker_stream_evict(self._h, len(row_ids), ids_c))

    @_lib.locked
    def stream_step(self, max_frames_now: int):
        """`qtts_talker_stream_step` on the open stream: (frame steps the stream has run, whether its stop condition has latched)."""
        total, fin = C.c_int32(0), C.c_int32(0)
        with torch.cuda.device(self.device), torch.cuda.stream(self._stream):
            _lib.check(self._lib.qtts_talker_stream_step(self._h, int(max_frames_now), C.byref(total), C.byref(fin), self._s()))
        return int(total.value), bool(fin.value)

    @_lib.locked
    def stream_close(self, tokens: Optional[torch.Tensor] = None) -> int:
        """`qtts_talker_stream_end`; returns the frame steps the stream ran.  `tokens`: optional int64 (B, max_row_tokens) device block
        that receives the codebook-0 tokens of every row's current occupant (-1 behind them)."""
        nf = C.c_int32(0)
        with torch.cuda.device(self.device), torch.cuda.stream(self._stream):
            _lib.check(self._lib.qtts_talker_stream_end(self._h, C.c_void_p(tokens.data_ptr()) if tokens is not None else None,
                                                        C.byref(nf), self._s()))
        torch.cuda.current_stream(self.device).wait_stream(self._stream)
        self._open = None
        return int(nf.value)

    def _refill_stream(self, *args, output_hidden_states: bool = False, packet_frames: int = 4, row_positions: bool = False, **kw):
        """The refill schedule, packet by packet (`generate_stream(..., schedule="refill")`; `generate(..., schedule="refill")` collects
        what this yields): any number of requests on `max_batch` rows.  The rows start with the requests of the longest prompts; the
        stream runs in packets of `packet_frames` frames; after each packet every row whose occupant gained frames or finished is
        reported in one `RefillPacket` (the new frames copied out, cut at the first eos in codebook 0 or at the request's limit), the
        finished rows are retired and every queued request that fits -- prompt no longer than the stream's position, position + its
        limit inside max_seq -- is admitted, longest prompt first, in one `stream_admit`.  When requests remain but none fits and every
        row has finished, the stream ends and a fresh one begins with the remainder.  Always runs on the per-row table (scalars are
        broadcast; seeds as in `_row_table`: a list is per request, one integer s gives request i the seed s + i, none draws fresh
        ones), so a request's codes do not depend on when or where it was admitted.  Closing the generator closes the stream;
        `last_refill` is filled either way.  Holds the engine lock while active.

        `row_positions=True` (`schedule="continuous"`): the stream carries per-row positions, so the fit test on the position is gone --
        after every packet every queued request for which a row is free is admitted, in queue order (a group whose padded length would
        push one of its members past max_seq is split into several `stream_admit` calls) -- and ONE stream serves the whole call, at
        full width: the opening group is the widest that fits (`_widest_opener`) and the remaining rows start as spare rows.
        `last_refill["max_row_len"]` is the largest row length seen.

        On an engine with a KV page pool (`kv_pages`) the continuous schedule is optimistic: rows take pages as they grow and nobody
        reserves a worst case.  Admission: after each packet, in queue order, only while the group's prompt pages fit AND one page per row
        that would then be running stays free (the watermark keeps a preempted request from being admitted straight into the next
        preemption; a pool that holds max_seq keys for every row can never run dry and admits like the static engine).  Before each `stream_step(packet_frames)`: while the pool cannot cover the step, the running request with the
        fewest frames (ties: the highest request index) is evicted (`stream_evict`) and returns to the FRONT of the queue; the only
        running row is never evicted, and the request with the most frames always keeps running, finishes and frees its pages, so the
        call terminates.  A re-admitted request starts again at frame 0: its first packet carries `first=True, restart=True`.  Its codes
        are the same as before (a request's draws depend on its seed and its own step only).  `last_refill` reports `pool_pages`,
        `peak_pages` and `preemptions`.  The other schedules on a pooled engine reserve their worst case when a stream begins.

        Width on a pooled engine: the opening group's prompts (the spare rows' copies of the first prompt included) must fit the pool,
        so the stream opens with at most `kv_pages // ceil(longest opening prompt / 16)` rows -- and a stream keeps its opening width
        for the whole call.  A pool that is tight against a long first prompt therefore serves the whole request list on that narrower
        stream, also after the long prompt has retired and its pages are free (`last_refill["occupancy"]` is measured against
        `max_batch` and shows it).  It costs throughput, never correctness; size the pool to at least
        `max_batch x ceil(longest prompt / 16)` pages to open at full width.

        The arguments are `_prepare`'s (its queue mode).  Every decision above is `refill.RefillPolicy`'s; this generator drives the
        engine with it and hands it what the engine reports."""
        if packet_frames < 1:
            raise ValueError("packet_frames must be >= 1")
        p = self._prepare(True, *args, **kw)
        pol = RefillPolicy(p.lens, [int(r.max_new_tokens) for r in p.rows], self.max_batch, self.max_seq, packet_frames, row_positions,
                           self.kv_pages)

        def group(idx, spare=0):
            """the requests `idx`, and `spare` spare rows behind them, as `stream_open` / `stream_admit` take a group"""
            idx = idx + idx[:1] * spare
            Tg = max(p.lens[i] for i in idx)
            tab = (_lib.RowSamplingC * len(idx))(*[p.rows[i] for i in idx])
            for k in range(len(idx) - spare, len(idx)):
                tab[k].max_new_tokens, tab[k].min_new_tokens = 1, 0
            wtab = (_lib.RowWarpersC * len(idx))(*[p.warp[i] for i in idx]) if p.warp is not None else None
            ptab = (_lib.RowProcessorsC * len(idx))(*[p.proc[i] for i in idx]) if p.proc is not None else None
            return p.emb[idx][:, p.T - Tg:], [Tg - p.lens[i] for i in idx], p.trail[idx], tab, wtab, ptab

        with self._lock:
            caps0 = self.stats()["graph_captures"]
            try:
                while pol.queue:
                    e, npd, tr, tab, wtab, ptab = group(*pol.open_stream())
                    codes, hidden = self.stream_open(e, npd, tr, p.pad, tab, p.max_new_tokens, p.eos, p.suppress, output_hidden_states,
                                                     row_positions, warpers=wtab, processors=ptab)
                    try:
                        while pol.active:
                            # (pooled: the engine's counts are read again after every eviction)
                            while pol.pooled and (victim := pol.victim(*self.stream_kv()[:2], self.stream_row_lens())) is not None:
                                self.stream_evict([victim])
                            self.stream_step(packet_frames)
                            unfinished, frames, kv_len = self.stream_rows()
                            yield RefillPacket([RefillRow(request=r.request, row=r.row, codes=codes[r.row, r.k0:r.k1].clone(), first=r.first,
                                                          last=r.last, restart=r.restart,
                                                          hidden=hidden[r.row, r.k0:r.k1].clone() if hidden is not None else None)
                                                for r in pol.reports(unfinished, frames)])
                            for row_ids, grp in pol.admissions(kv_len, self.stream_kv()[1] if pol.tight else None):
                                e, npd, tr, tab, wtab, ptab = group(grp)
                                self.stream_admit(row_ids, e, npd, tr, tab, warpers=wtab, processors=ptab)
                    finally:
                        pol.stream_closed(self.stats(), self.stream_close())
            finally:
                self.last_refill = pol.finish(self.stats()["graph_captures"] - caps0)

    _widest_opener = staticmethod(widest_opener)

    def _generate_refill(self, inputs_embeds: torch.Tensor, *args, eos_token_id: Optional[int] = None, output_hidden_states: bool = True,
                         **kw) -> TalkerGenerateOutput:
        """`generate(..., schedule="refill")`: the packets of `_refill_stream` (its arguments and schedule) collected per request.
        Returns the requests in the order given, in `generate`'s structure: codes (N, F, G) with eos in codebook 0 behind a request's
        last frame, tokens (N, F + 1)."""
        c, dev = self.config, self.device
        eos = c.codec_eos_token_id if eos_token_id is None else int(eos_token_id)
        N, G, H = int(inputs_embeds.shape[0]), c.num_code_groups, c.hidden_size
        parts, hparts = [[] for _ in range(N)], [[] for _ in range(N)]
        for packet in self._refill_stream(inputs_embeds, *args, eos_token_id=eos, output_hidden_states=output_hidden_states, **kw):
            for e in packet.rows:
                if e.restart:         # a preempted request starts again at frame 0: what it had delivered is replayed
                    parts[e.request], hparts[e.request] = [], []
                parts[e.request].append(e.codes)
                hparts[e.request].append(e.hidden)
        out_codes = [torch.cat(p) for p in parts]
        F = max([1] + [int(x.shape[0]) for x in out_codes])
        codes_all = torch.zeros(N, F, G, dtype=torch.int64, device=dev)
        codes_all[:, :, 0] = eos
        hidden_all = torch.zeros(N, F, H, dtype=torch.float32, device=dev) if output_hidden_states else None
        tokens = torch.full((N, F + 1), eos, dtype=torch.int64, device=dev)
        for i in range(N):
            n = int(out_codes[i].shape[0])
            codes_all[i, :n] = out_codes[i]
            tokens[i, :n] = out_codes[i][:, 0]
            if hidden_all is not None:
                hidden_all[i, :n] = torch.cat(hparts[i])
        return TalkerGenerateOutput(codes=codes_all, hidden=hidden_all, tokens=tokens, n_frames=F)

    @_lib.locked
    def sampler_class(self):
        """`qtts_talker_sampler_class`: (talker, code predictor) sampler kernels of the open stream or the last call -- 0 launch
        constants (a scalar call), 1 `sample_kernel_v2`, 2 `sample_kernel`, 3 `sample_warp_kernel` (talker only)."""
        a, b = C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.qtts_talker_sampler_class(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    @_lib.locked
    def debug_logits(self) -> torch.Tensor:
        out = torch.empty(self.max_batch, self.config.vocab_size, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.qtts_talker_debug_logits(self._h, C.c_void_p(out.data_ptr()), self._s()))
            self._stream.synchronize()
        return out

    @_lib.locked
    def debug_cp_logits(self) -> torch.Tensor:
        """(num_code_groups - 1, B, cp_vocab): the code predictor's raw logits of the last frame step that ran, every pass; B is the batch
        of the last call (the engine packs pass j at j * B * cp_vocab with that live B, not with max_batch)."""
        B = getattr(self, "_live_batch", self.max_batch)
        out = torch.empty(self.config.num_code_groups - 1, B, self.config.cp_vocab_size, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.qtts_talker_debug_cp_logits(self._h, C.c_void_p(out.data_ptr()), self._s()))
            self._stream.synchronize()
        return out
