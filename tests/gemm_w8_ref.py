"""What the FP8 weight-stream GEMM tests share (tests/test_gemm_w8_gpu.py, tests/test_gemm_w8_rows_gpu.py): the
weights with their dequantised float64 image, the SwiGLU reference, the three row bands of the stream and the launch
counters that say which kernel family a call ran."""
import functools

import torch

# band (the most rows its entry serves) -> how a PackedLinearW8 is sent there, the C-ABI entry, the entry's own launch
# kind and the row counts its tests run: for 64 and 128 one row into a row block, full row blocks and the last one
BANDS = {
    16: dict(stream_rows=16, rows_rb=None, entry="fo_gemm_w8", kind="gemm_w8", rows=(1, 8, 16)),
    64: dict(stream_rows=64, rows_rb=(2, 3, 4), entry="fo_gemm_w8_rows", kind="gemm_w8_rows",
             rows=(17, 32, 33, 48, 49, 64)),
    128: dict(stream_rows=128, rows_rb=tuple(range(2, 9)), entry="fo_gemm_w8_rows128", kind="gemm_w8_rows128",
              rows=(65, 80, 81, 112, 113, 128)),
}
W8_KINDS = ("gemm_w8", "gemm_w8_xs", "gemm_w8_rows", "gemm_w8_rows128")
BF16_KINDS = ("gemm_xsk", "gemm_rows")   # what the bf16 image runs at 17..128 rows


@functools.lru_cache(maxsize=None)
def _weight(N, K, seed):
    """(bf16 weight, its dequantised FP8 image as float64), on the CPU, shared between the tests."""
    from fo.quant import quantize_rows_e4m3
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    return w, quantize_rows_e4m3(w)[2].double()


@functools.lru_cache(maxsize=None)
def _swiglu_ref(N, K, M, seed):
    (_, gdq), (_, udq) = _weight(N, K, 1), _weight(N, K, 2)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(seed))
    return x, torch.nn.functional.silu(x.double() @ gdq.t()) * (x.double() @ udq.t())


def lin(dev, band, w, up=None):
    """PackedLinearW8 of w (and the SwiGLU up) that sends every call of up to `band` rows to the FP8 kernels,
    whatever the measured dispatch policy keeps on the image."""
    from fo.ops import PackedLinearW8
    b = BANDS[band]
    p = PackedLinearW8(w.to(dev), swiglu_up=None if up is None else up.to(dev), stream_rows=b["stream_rows"])
    if b["rows_rb"] is not None:
        p.rows_rb = b["rows_rb"]
    return p


def counts():
    from fo import ops
    c = ops.launch_counts()
    return {k: c[k] for k in W8_KINDS + BF16_KINDS}


def assert_rose(before, band, n, free=()):
    """Since `before` = counts(), the band's own kind rose by n and no other kind moved (but those in `free`)."""
    now, own = counts(), BANDS[band]["kind"]
    want = {k: before[k] + (n if k == own else 0) for k in now if k not in free}
    assert {k: now[k] for k in want} == want
