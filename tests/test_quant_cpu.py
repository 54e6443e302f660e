"""The weight-only FP8 model on the host: the reference quantiser (fo.quant, the definition of mlp_weights="fp8") and
fo_gemm_w8's argument checks, which refuse before the library touches the device.  No GPU needed."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("FO_LIB_PATH") or os.path.join(ROOT, "freeze-omni_amd", "fo", "libfo_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libfo_hip.so not built (run __graft_entry__.build())")

FAKE = 1 << 20   # dummy device addresses: never dereferenced by a refused call


def edge_weight():
    """40 x 96 bf16: random rows of mixed magnitude, row 3 all zero, row 5 with amax exactly 448 * 2^-12, row 6 with
    the next bf16 above that, row 7 / 8 on e4m3 rounding ties (amax 256 so e = 0: 17, 19, 0.5 * 2^-9, 1.5 * 2^-9 and
    their negatives lie midway between two codes)."""
    g = torch.Generator().manual_seed(11)
    w = torch.randn(40, 96, generator=g) * torch.logspace(-6, 3, 40, base=2.0)[:, None]
    w[3] = 0
    w[5] = w[5].clamp(-0.05, 0.05)
    w[5, 17] = 448 * 2.0 ** -12
    w[6] = w[5]
    w[6, 17] = -(448 + 2) * 2.0 ** -12      # 1.75 * 2^-4 plus one bf16 ulp (2^-11)
    ties = torch.tensor([17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10, 34.0, 38.0, 27.0, 29.0])
    w[7] = torch.cat([ties, -ties]).repeat(6)
    w[7, 0] = 256.0
    w[8] = -w[7]
    return w.to(torch.bfloat16)


def test_reference_quantiser_properties():
    from fo.quant import quantize_rows_e4m3
    w = edge_weight()
    q, e, w_dq = quantize_rows_e4m3(w)
    assert q.dtype == torch.uint8 and q.shape == w.shape and e.shape == (40,) and w_dq.dtype == torch.bfloat16
    codes = q.view(torch.float8_e4m3fn).float()
    assert torch.isfinite(codes).all() and codes.abs().max() <= 448
    # q * 2^e is exactly a bf16 value: the image survives the round trip through bf16 unchanged
    exact = torch.ldexp(codes.double(), e[:, None])
    assert torch.equal(w_dq.double(), exact)
    assert torch.equal(w_dq.float().to(torch.bfloat16), w_dq)
    amax = w.float().abs().amax(1)
    nz = amax > 0
    assert e[3] == 0 and not codes[3].any() and not w_dq[3].any()
    # e is minimal: amax fits under 448 at e and would not at e - 1
    assert (torch.ldexp(amax, -e)[nz] <= 448).all()
    assert (torch.ldexp(amax, 1 - e)[nz] > 448).all()
    # ... so every non-zero row's largest code lies in the top binade.  (amax * 2^-e in (224, 232] rounds to the
    # code 224 itself -- row 6, one bf16 ulp above 448 * 2^-12, is 225 -> 224 -- so the bound is inclusive.)
    top = codes.abs().amax(1)
    assert (top[nz] >= 224).all() and (top[nz & (torch.ldexp(amax, -e) > 232)] > 224).all()
    assert e[5] == -12 and top[5] == 448 and e[6] == -11 and top[6] == 224
    # ties go to the even code (e = 0 in rows 7 / 8)
    assert e[7] == 0 and e[8] == 0
    want = torch.tensor([16.0, 20.0, 0.0, 2.0 ** -8, 32.0, 40.0, 28.0, 28.0])
    assert torch.equal(codes[7, 8:16], -want) and torch.equal(codes[7, 16:24], want)
    assert torch.equal(codes[8], -codes[7])
    # the nearest code everywhere: no other e4m3 value is closer to W * 2^-e
    grid = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    grid = grid[torch.isfinite(grid)]
    scaled = torch.ldexp(w.float(), -e[:, None])
    best = (scaled[..., None] - grid).abs().amin(-1)
    assert torch.equal((scaled - codes).abs(), best)


def test_quantiser_is_idempotent_in_value():
    """Quantising the dequantised weight gives the same weight (a second engine built on engine.src is the same
    model), and a float32 copy of a weight quantises as the bf16 one."""
    from fo.quant import quantize_rows_e4m3
    w = edge_weight()
    _, _, w_dq = quantize_rows_e4m3(w)
    assert torch.equal(quantize_rows_e4m3(w_dq)[2], w_dq)
    assert torch.equal(quantize_rows_e4m3(w.float())[2], w_dq)


def test_packed_order():
    from fo.quant import pack_codes, pack_scales
    q = (torch.arange(20 * 96) % 251).to(torch.uint8).view(20, 96)
    p = pack_codes(q).view(2, 2, 64, 16)           # [tile][code step][lane][byte]
    for n, k in ((0, 0), (3, 9), (15, 63), (17, 64), (19, 95), (16, 40)):
        assert p[n // 16, k // 64, 16 * (k % 32 // 8) + n % 16, 8 * (k % 64 // 32) + k % 8] == q[n, k]
    assert not p[1, :, 4:16].any() and not p[1, :, 20:32].any()      # rows 20..31: zero codes
    assert not p[:, 1, :, 8:].any()                                   # columns 96..127: zero codes
    gu = pack_codes(q, 1, 2, pack_codes(q, 0, 2, torch.zeros(4 * 2048, dtype=torch.uint8))).view(4, 2048)
    assert torch.equal(gu[0], gu[1]) and torch.equal(gu[2], gu[3]) and torch.equal(gu[2], p[1].reshape(-1))
    s = pack_scales(torch.arange(20, dtype=torch.int32) - 10)
    assert s.shape == (32,) and s[0] == 2.0 ** -10 and s[19] == 2.0 ** 9 and (s[20:] == 1).all()


def _w8(lib, M=8, K=128, N=64, scale=FAKE, ntiles=None, swiglu=0):
    nt = (N + 15) // 16 * (2 if swiglu else 1) if ntiles is None else ntiles
    return lib.fo_gemm_w8(FAKE, K, M, K, FAKE, scale, nt, N, swiglu, FAKE, N, 0, None, 0, None, None, 0,
                          ctypes.c_float(0.0), None, None, None, None, None)


@needs_lib
def test_gemm_w8_refuses_before_touching_the_device():
    from fo import _lib
    lib, err = _lib.load(), _lib.last_error
    assert _w8(lib, M=17) == -2 and "M=17" in err(), err()
    assert _w8(lib, K=100) == -2 and "K=100" in err() and "multiple of 32" in err(), err()
    assert _w8(lib, scale=None) == -2 and "scale" in err(), err()
    assert _w8(lib, N=40, swiglu=1, ntiles=5) == -2 and "ntiles=5" in err() and "swiglu" in err(), err()
    assert _w8(lib, N=40, ntiles=2) == -2 and "ntiles=2" in err(), err()          # not the weight's tile count
    # a producer needs a plain launch, and its yg the next norm's gamma
    assert lib.fo_gemm_w8(FAKE, 128, 8, 128, FAKE, FAKE, 8, 64, 1, FAKE, 64, 0, None, 0, None, None, 0,
                          ctypes.c_float(0.0), FAKE, FAKE, FAKE, None, None) == -2 and "sout" in err(), err()
    assert lib.fo_quant_w8(FAKE, 1, 16, 64, 32, FAKE, FAKE, None, 0, 1, None) == -2 and "ldw=32" in err(), err()
    assert lib.fo_quant_w8_bytes(3584, 18944) == 224 * 296 * 1024 and lib.fo_quant_w8_bytes(20, 96) == 2 * 2 * 1024


@needs_lib
def test_launch_kinds_cover_the_w8_counters():
    from fo import ops
    assert ops.LAUNCH_KINDS.index("gemm_w8") == 20 and ops.LAUNCH_KINDS.index("gemm_w8_xs") == 21
    assert len(ops.LAUNCH_KINDS) <= ops._lib.load().fo_launch_counts(None, 0)


def test_cli_option_defaults_to_bf16():
    import importlib
    inf, srv = importlib.import_module("bin.inference"), importlib.import_module("bin.server")
    base = ["--model_path", "m", "--llm_path", "l", "--input_wav", "i.wav", "--output_wav", "o.wav"]
    assert inf.get_args(base).llm_mlp_weights == "bf16"
    assert inf.get_args(base + ["--llm_mlp_weights", "fp8"]).llm_mlp_weights == "fp8"
    with pytest.raises(SystemExit):
        inf.get_args(base + ["--llm_mlp_weights", "int8"])
    assert srv.get_parser().parse_args([]).llm_mlp_weights is None      # the config's value, else bf16
    assert srv.get_parser().parse_args(["--llm_mlp_weights", "fp8"]).llm_mlp_weights == "fp8"
