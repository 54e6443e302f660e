"""Qwen2 backbone of AudioLLM on the MI355X kernels (frozen LLM, per-session paged KV).

Reference: AudioLLM._llm_forward_core -> Qwen2Model (models/audioLLM.py:479-484), the dialog-state
head (models/audioLLM.py:486-527) and the sampler _post_decode (models/audioLLM.py:431-477).
"""
import numpy as np
import torch

from . import ops, tables
from .kv import BatchMeta, KVPool, KVSeq
from .ops import F32, I32, QUANT_LINEAR, PackedLinear
from .quant import check_format
from .stack import DecoderStack
from .weights import ReceiveSource


class LLMEngine:
    def __init__(self, src, llm_cfg, device, head_src=None, kv_tokens=65536, page_size=16, max_pos=None,
                 mlp_weights="bf16", mlp_rows=16, kv_dtype="fp32", lm_head_weights="bf16", attn_weights="bf16",
                 rows_x="fp32"):
        """rows_x: "fp32" (default) or "bf16" -- the GEMM inputs of the 65..128-row forwards (the 5..8-chunk listen
        groups at 8 sessions, a 65..128-row prefill) rounded to bf16, the reference's autocast arithmetic (DESIGN
        §5.12; DecoderStack rows_x).  Steps of <= 64 rows are bit for bit what they are without it.
        mlp_weights: "bf16" (default), "fp8", "mxfp4" or "mxfp6" -- mlp.{gate,up,down}_proj.weight of every layer
        under that weight-only format, and mlp_rows, the most rows of a step that stream
        the codes: DecoderStack's options of the same names.
        attn_weights: "bf16" (default), "fp8" or "mxfp4" -- self_attn.{q,k,v,o}_proj.weight of every layer under
        weight-only FP8 / MXFP4 (DecoderStack attn_weights): steps of <= 16 rows stream the codes where
        ops.ATTN_POLICY says so, everything else runs the exact bf16 image.  The biases are untouched.
        lm_head_weights: "bf16" (default), "fp8", "mxfp4" or "mxfp6" -- lm_head.weight under weight-only FP8 / MXFP4 /
        MXFP6: calls of <= 16 rows stream the codes where ops.HEAD_POLICY (ops.W6_POLICY for
        MXFP6) says so, every other call runs the exact bf16 image.  embed_tokens is never quantised.  Over a
        ReceiveSource the head's storages are allocated and nothing is quantised (a replica whose weights arrive by
        broadcast fills codes, scales and image).
        kv_dtype: "fp32" (default), "bf16" or "e4m3" -- the paged KV's element.  "bf16" (DESIGN §5.6): K / V rounded
        once to bf16 as they are appended and read as bf16 by the attention; kv_tokens keeps meaning tokens (half the
        bytes).  "e4m3" (DESIGN §5.11): e4m3fn codes with one power-of-two scale per (token, kv head), quantised by a
        launch of its own after the q|k|v projection and decoded in registers by the attention (0.26 of the bytes)."""
        if kv_dtype not in ("fp32", "bf16", "e4m3"):
            raise ValueError(f'kv_dtype must be "fp32", "bf16" or "e4m3", got {kv_dtype!r}')
        self.mlp_weights = check_format("mlp_weights", mlp_weights)
        self.lm_head_weights = check_format("lm_head_weights", lm_head_weights)
        self.attn_weights = check_format("attn_weights", attn_weights)
        self.rows_x = check_format("llm_rows_x", rows_x)
        self.mlp_rows = mlp_rows
        self.kv_dtype = kv_dtype
        c = llm_cfg
        self.device = torch.device(device)
        self.D, self.V = c["hidden_size"], c["vocab_size"]
        self.H, self.KVH = c["num_attention_heads"], c["num_key_value_heads"]
        self.hd = self.D // self.H
        self.eps = c["rms_norm_eps"]
        max_pos = max_pos or min(c.get("max_position_embeddings", 32768), 32768)
        cos, sin = tables.rope_tables(c["rope_theta"], self.hd, max_pos, round_fp16=True)
        self.rope = (cos.to(self.device), sin.to(self.device))
        n_pages = (kv_tokens + page_size - 1) // page_size
        self.pool = KVPool(c["num_hidden_layers"], self.KVH, self.hd, n_pages, page_size, self.device,
                           dtype={"fp32": torch.float32, "bf16": torch.bfloat16, "e4m3": torch.float8_e4m3fn}[kv_dtype])
        self.stack = DecoderStack(src, "model.layers.", c["num_hidden_layers"], self.D, self.H, self.KVH, self.eps,
                                  True, self.rope, self.pool, first_fp16=True, mlp_weights=mlp_weights,
                                  mlp_rows=mlp_rows, attn_weights=attn_weights, rows_x=rows_x)
        self.embed_tokens = src.get("model.embed_tokens.weight", torch.bfloat16)
        self.norm = src.get("model.norm.weight")
        if lm_head_weights == "bf16":
            self.lm_head = PackedLinear(src.get("lm_head.weight", torch.bfloat16))
        else:
            self.lm_head = QUANT_LINEAR[lm_head_weights](src.get("lm_head.weight", torch.bfloat16),
                                                         receive=isinstance(src, ReceiveSource), kind="head")
        hs = head_src or src
        self.head_w = hs.get("predictor_head.weight") if "predictor_head.weight" in hs else None
        self.head_b = hs.get("predictor_head.bias") if self.head_w is not None else None

    @property
    def weight_bytes(self):
        return self.stack.weight_bytes

    def head_code_bytes(self, fmt):
        """The head's codes and scales of format `fmt`, held beside its bf16 image (0 unless lm_head_weights is fmt)."""
        return getattr(self.lm_head, ops.QUANT_FORMATS[fmt].nbytes_attr, 0)

    mlp_fp8_bytes = property(lambda self: self.stack.code_bytes("mlp", "fp8"))
    mlp_fp4_bytes = property(lambda self: self.stack.code_bytes("mlp", "mxfp4"))
    mlp_fp6_bytes = property(lambda self: self.stack.code_bytes("mlp", "mxfp6"))
    attn_fp8_bytes = property(lambda self: self.stack.code_bytes("attn", "fp8"))
    attn_fp4_bytes = property(lambda self: self.stack.code_bytes("attn", "mxfp4"))
    lm_head_fp8_bytes = property(lambda self: self.head_code_bytes("fp8"))
    lm_head_fp4_bytes = property(lambda self: self.head_code_bytes("mxfp4"))
    lm_head_fp6_bytes = property(lambda self: self.head_code_bytes("mxfp6"))

    def new_seq(self):
        return KVSeq(self.pool)

    def embed(self, ids, out=None, round_fp16=False):
        if torch.is_tensor(ids):
            ids_d = ids.to(device=self.device, dtype=I32)
        else:
            ids_d = ops.h2d(np.asarray(list(ids), np.int32), self.device)
        return ops.gather_rows(self.embed_tokens, ids_d, out=out, round_fp16=round_fp16)

    def forward(self, x, entries):
        """x: fp32 [T, D] input embeds (already rounded to fp16 values, models/audioLLM.py:338,410);
        entries: list of (KVSeq, n_tokens).  Returns (final-normed hidden [T, D], BatchMeta)."""
        meta = BatchMeta([(s, n, s.length, True) for s, n in entries], self.device, gqa=self.H // self.KVH,
                         rows=ops.attn_item_rows(self.hd))
        self.stack.forward(x, meta)
        ops.rmsnorm(x, self.norm, self.eps, out=x)
        return x, meta

    def state_probs(self, hidden, rows):
        """softmax over the first 3 predictor-head logits at the given rows -> device [S, 3]."""
        rows_d = rows if torch.is_tensor(rows) else ops.h2d(np.asarray(list(rows), np.int32), self.device)
        out = torch.empty(rows_d.numel(), 3, dtype=F32, device=self.device)
        return ops.state_head(hidden, rows_d, self.head_w, self.head_b, out)

    def logits(self, hidden, rows):
        rows_d = rows if torch.is_tensor(rows) else torch.tensor(list(rows), dtype=I32).to(self.device)
        h = ops.gather_rows(hidden, rows_d)
        return self.lm_head(h)
