"""Which entry a quantised linear layer launches (ops.PackedLinearQuant through PackedLinearW8 / W4 / W6): every format
x GEMM x stream_rows x row count, under the committed policy and with `stream` / `rows_rb` forced on, against a literal
table written from the three per-format classes this one class replaced.  The numerics of every entry are pinned by its
own test module (test_gemm_w*_gpu.py, test_gemm_head_gpu.py); this one pins the routing alone, on the smallest shapes
those modules run each entry at.  Also: a receive-only layer is laid out like a quantising one."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = (1, 16, 17, 64, 65, 128, 129)
HEAD_K = 3584

IMG = "fo_gemm"                       # the bf16 image's entry: "runs the image"
G8, R8, B8, H8 = "fo_gemm_w8", "fo_gemm_w8_rows", "fo_gemm_w8_rows128", "fo_gemm_w8_head"
G4, R4, H4 = "fo_gemm_w4", "fo_gemm_w4_rows", "fo_gemm_w4_head"
G6, H6 = "fo_gemm_w6", "fo_gemm_w6_head"

# (format, GEMM, stream_rows) -> (the entries at ROWS under the committed policy, the same with stream = True and
# rows_rb = (2, ..., 8)).  Policy: W8_ROWS_POLICY gate/up (2, 3, 4), down (2,); W4_ROWS_POLICY gate/up (2, 3, 4), down
# (2, 3); every <= 16-row MLP GEMM and head streams; no attention output does (ATTN_POLICY o: False).
WANT = {
    ("fp8", "gate_up", 16):    ((G8, G8, IMG, IMG, IMG, IMG, IMG), (G8, G8, IMG, IMG, IMG, IMG, IMG)),
    ("fp8", "gate_up", 64):    ((G8, G8, R8, R8, IMG, IMG, IMG), (G8, G8, R8, R8, IMG, IMG, IMG)),
    ("fp8", "gate_up", 128):   ((G8, G8, R8, R8, IMG, IMG, IMG), (G8, G8, R8, R8, B8, B8, IMG)),
    ("fp8", "down", 16):       ((G8, G8, IMG, IMG, IMG, IMG, IMG), (G8, G8, IMG, IMG, IMG, IMG, IMG)),
    ("fp8", "down", 64):       ((G8, G8, R8, IMG, IMG, IMG, IMG), (G8, G8, R8, R8, IMG, IMG, IMG)),
    ("fp8", "down", 128):      ((G8, G8, R8, IMG, IMG, IMG, IMG), (G8, G8, R8, R8, B8, B8, IMG)),
    ("fp8", "head_k", 16):     ((H8, H8, IMG, IMG, IMG, IMG, IMG), (H8, H8, IMG, IMG, IMG, IMG, IMG)),
    ("fp8", "head", 16):       ((G8, G8, IMG, IMG, IMG, IMG, IMG), (G8, G8, IMG, IMG, IMG, IMG, IMG)),
    ("fp8", "attn_o", 16):     ((IMG, IMG, IMG, IMG, IMG, IMG, IMG), (G8, G8, IMG, IMG, IMG, IMG, IMG)),
    ("mxfp4", "gate_up", 16):  ((G4, G4, IMG, IMG, IMG, IMG, IMG), (G4, G4, IMG, IMG, IMG, IMG, IMG)),
    ("mxfp4", "gate_up", 64):  ((G4, G4, R4, R4, IMG, IMG, IMG), (G4, G4, R4, R4, IMG, IMG, IMG)),
    ("mxfp4", "down", 16):     ((G4, G4, IMG, IMG, IMG, IMG, IMG), (G4, G4, IMG, IMG, IMG, IMG, IMG)),
    ("mxfp4", "down", 64):     ((G4, G4, R4, IMG, IMG, IMG, IMG), (G4, G4, R4, R4, IMG, IMG, IMG)),
    ("mxfp4", "head_k", 16):   ((H4, H4, IMG, IMG, IMG, IMG, IMG), (H4, H4, IMG, IMG, IMG, IMG, IMG)),
    ("mxfp4", "head", 16):     ((G4, G4, IMG, IMG, IMG, IMG, IMG), (G4, G4, IMG, IMG, IMG, IMG, IMG)),
    ("mxfp4", "attn_o", 16):   ((IMG, IMG, IMG, IMG, IMG, IMG, IMG), (G4, G4, IMG, IMG, IMG, IMG, IMG)),
    ("mxfp6", "gate_up", 16):  ((G6, G6, IMG, IMG, IMG, IMG, IMG), (G6, G6, IMG, IMG, IMG, IMG, IMG)),
    ("mxfp6", "down", 16):     ((G6, G6, IMG, IMG, IMG, IMG, IMG), (G6, G6, IMG, IMG, IMG, IMG, IMG)),
    ("mxfp6", "head_k", 16):   ((H6, H6, IMG, IMG, IMG, IMG, IMG), (H6, H6, IMG, IMG, IMG, IMG, IMG)),
    ("mxfp6", "head", 16):     ((G6, G6, IMG, IMG, IMG, IMG, IMG), (G6, G6, IMG, IMG, IMG, IMG, IMG)),
}
# [N, K]: the ragged plain and SwiGLU shapes of the per-entry tests ((3 | 17, 100, 96), (5 | 20, 200, 160)), the MXFP6
# head test's 80 columns at HEAD_K
SHAPE = {"gate_up": (200, 160), "down": (100, 96), "head_k": (80, HEAD_K), "head": (100, 96), "attn_o": (100, 96)}


def _weight(N, K, seed):
    return (torch.randn(N, K, generator=torch.Generator().manual_seed(seed)) / K ** 0.5).to(torch.bfloat16)


def _layer(dev, fmt, gemm, stream_rows=16, receive=False):
    from fo import ops
    cls = {"fp8": ops.PackedLinearW8, "mxfp4": ops.PackedLinearW4, "mxfp6": ops.PackedLinearW6}[fmt]
    N, K = SHAPE[gemm]
    kw = {"receive": receive}
    if gemm == "gate_up":
        kw["swiglu_up"] = _weight(N, K, 2).to(dev)
    if gemm in ("head_k", "head"):
        kw["kind"] = "head"
    if gemm == "attn_o":
        kw["kind"] = "attn_o"
    if stream_rows != 16:
        kw["stream_rows"] = stream_rows
    return cls(_weight(N, K, 1).to(dev), **kw)


@pytest.fixture
def recorder(monkeypatch):
    """ops._lib.call wrapped: the entry names called, in order; every call goes through."""
    from fo import ops
    names, call = [], ops._lib.call

    def rec(name, *a):
        names.append(name)
        return call(name, *a)

    monkeypatch.setattr(ops._lib, "call", rec)
    return names


@pytest.mark.parametrize("fmt,gemm,stream_rows", list(WANT), ids=["-".join(map(str, k)) for k in WANT])
def test_entry_called(dev, recorder, fmt, gemm, stream_rows):
    from fo import ops
    assert HEAD_K == ops.HEAD_K
    lin = _layer(dev, fmt, gemm, stream_rows)
    assert type(lin).__mro__[1] is ops.PackedLinearQuant and lin.fmt == fmt and lin.stream_rows == stream_rows
    N, K = SHAPE[gemm]
    x = torch.randn(ROWS[-1], K, generator=torch.Generator().manual_seed(3)).to(dev)
    policy, forced = WANT[fmt, gemm, stream_rows]
    for want in (policy, forced):
        for M, entry in zip(ROWS, want):
            del recorder[:]
            y = lin(x[:M])
            assert recorder == [entry], (fmt, gemm, stream_rows, M, want is forced, recorder)
            assert lin.streams(M) == (entry != IMG) and y.shape == (M, N)
        lin.stream, lin.rows_rb = True, tuple(range(2, 9))      # the second pass: forced on
    torch.cuda.synchronize()


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4", "mxfp6"])
def test_head_entry_is_plain(dev, recorder, fmt):
    """A residual sends a K = HEAD_K head to the image (its entry has no epilogue); a head of another K keeps it on the
    general form."""
    for gemm, want in (("head_k", IMG), ("head", WANT[fmt, "head", 16][0][0])):
        lin = _layer(dev, fmt, gemm)
        N, K = SHAPE[gemm]
        out = torch.zeros(8, N, device=dev)
        del recorder[:]
        lin(torch.randn(8, K).to(dev), out=out, residual=True)
        assert recorder == [want], (fmt, gemm, recorder)
    torch.cuda.synchronize()


def _shapes(obj):
    from fo.replica import frozen_tensors
    return [(tuple(t.shape), t.dtype) for t in frozen_tensors(obj)]


@pytest.mark.parametrize("gemm", ["gate_up", "down", "head_k"])
@pytest.mark.parametrize("fmt", ["fp8", "mxfp4", "mxfp6"])
def test_receive_only_layer_is_laid_out_like_a_quantising_one(dev, fmt, gemm):
    a, b = _layer(dev, fmt, gemm), _layer(dev, fmt, gemm, receive=True)
    assert type(a) is type(b) and list(vars(a)) == list(vars(b))
    keys = list(vars(a))
    assert keys.index("q") < keys.index("scales") < keys.index("bf16")
    assert _shapes(a) == _shapes(b) and len(_shapes(a)) == 3       # codes, scales, the image
    assert (a.stream, a.rows_rb, a.stream_rows, a.kind) == (b.stream, b.rows_rb, b.stream_rows, b.kind)
    assert getattr(a, {"fp8": "fp8_nbytes", "mxfp4": "fp4_nbytes", "mxfp6": "fp6_nbytes"}[fmt]) > 0
    assert sorted((a.fp8_nbytes, a.fp4_nbytes, a.fp6_nbytes))[:2] == [0, 0]


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_receive_only_qkv_is_laid_out_like_a_quantising_one(dev, fmt):
    from fo.ops import PackedQKVQuant
    hd, N, K = 32, 128, 128                                         # H = 2, KVH = 1 (test_gemm_qkv_quant_gpu's hd32)
    w, bias = _weight(N, K, 5).to(dev), torch.randn(N).to(dev)
    a, b = PackedQKVQuant(w, bias, hd, fmt), PackedQKVQuant(w, bias, hd, fmt, receive=True)
    assert list(vars(a)) == list(vars(b)) and _shapes(a) == _shapes(b) and len(_shapes(a)) == 4   # ... and the bias
    assert a.stream == b.stream and (a.fp8_nbytes > 0) == (fmt == "fp8") and (a.fp4_nbytes > 0) == (fmt == "mxfp4")
    assert a.fp6_nbytes == 0
