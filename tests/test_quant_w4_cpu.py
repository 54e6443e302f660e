"""The weight-only MXFP4 model on the host: the reference quantiser (fo.quant, the definition of mlp_weights="mxfp4"),
its packed order against the layout text of include/fo_hip.h, and fo_gemm_w4 / fo_quant_w4's argument checks, which
refuse before the library touches the device.  No GPU needed."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("FO_LIB_PATH") or os.path.join(ROOT, "freeze-omni_amd", "fo", "libfo_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libfo_hip.so not built (run __graft_entry__.build())")

FAKE = 1 << 20   # dummy device addresses: never dereferenced by a refused call
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
TIES = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
TIES_TO = torch.tensor([0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0])


def edge_weight_w4():
    """20 x 96 (N no multiple of 16, K no multiple of 128), every value a bf16: random rows of mixed magnitude and
      row 3, block 1: all zero;
      row 4: block maxima exactly 6 * 2^-3, exactly 3 * 2^5 (mantissa 1.5: not above it) and the next bf16 above 3 * 2^5;
      row 5: every rounding tie and its negative at block exponent 0 (block 0, maximum 6) and at -4 (block 1, maximum
             6 * 2^-4), and in block 0 a -0.1 that rounds to zero with its sign kept;
      row 6, block 0: magnitudes below the clamp e >= -125 (maximum 1.5 * 2^-126 -> 0.75 -> 1, and fp32 denormals)."""
    g = torch.Generator().manual_seed(13)
    w = torch.randn(20, 96, generator=g) * torch.logspace(-8, 4, 20, base=2.0)[:, None]
    w[3, 32:64] = 0
    w[4] = w[4].clamp(-0.3, 0.3)
    w[4, 32:] *= 100
    w = w.to(torch.bfloat16).float()
    w[4, 7] = 6 * 2.0 ** -3
    w[4, 40] = -3 * 2.0 ** 5
    w[4, 70] = (3 + 2.0 ** -6) * 2.0 ** 5            # 1.5 * 2^6 plus one bf16 ulp
    both = torch.cat([TIES, -TIES])
    w[5, :32] = torch.cat([both, both, torch.tensor([6.0, -0.125, 0.125, -0.0])])
    w[5, 32:64] = torch.cat([both, both, torch.tensor([6.0, -0.125, 0.125, 0.0])]) * 2.0 ** -4
    w[6, :32] = 0
    w[6, :6] = torch.tensor([1.5 * 2.0 ** -126, -0.75 * 2.0 ** -126, 2.0 ** -130, -2.0 ** -127, 2.0 ** -126, -2.0 ** -133])
    wb = w.to(torch.bfloat16)
    assert torch.equal(wb.float().view(torch.int32), w.view(torch.int32))       # bf16 values as written
    return wb


def _decode(q):
    mag = GRID[(q & 7).long()]
    return torch.where((q & 8) != 0, -mag, mag)


def test_reference_quantiser_properties():
    from fo.quant import block_exponents, quantize_blocks_e2m1
    g = torch.Generator().manual_seed(2)
    for w in (edge_weight_w4(), torch.randn(48, 256, generator=g), (torch.rand(33, 64, generator=g) - 0.5) * 1e-3):
        N, K = w.shape
        q, e, w_dq = quantize_blocks_e2m1(w)
        assert q.dtype == torch.uint8 and q.shape == (N, K) and q.max() < 16
        assert e.dtype == torch.int32 and e.shape == (N, K // 32) and w_dq.dtype == torch.bfloat16
        assert torch.equal(e, block_exponents(w))
        ek = e.repeat_interleave(32, dim=1)
        # W' = q * 2^e exactly, and exactly a bf16 value
        exact = torch.ldexp(_decode(q).double(), ek)
        assert torch.equal(w_dq.double(), exact)
        assert torch.equal(w_dq.float().to(torch.bfloat16), w_dq)
        nz = w_dq != 0
        assert (w_dq[nz].float().abs() >= 2.0 ** -126).all()          # every non-zero W' is a normal bf16
        # the sign bit is the weight's, also where the magnitude rounded to zero
        assert torch.equal((q & 8) != 0, torch.signbit(w.float()))
        # scaled block maxima in (3, 6] (blocks above the clamp; an all-zero block has e = 0)
        amax = w.float().abs().view(N, K // 32, 32).amax(2)
        sm = torch.ldexp(amax.double(), -e)
        free = (amax > 0) & (e > -125)
        assert (sm[free] > 3).all() and (sm[free] <= 6).all()
        assert (e[amax == 0] == 0).all() and (e >= -125).all()
        assert (sm[(amax > 0) & (e == -125)] <= 6).all()
        # the nearest grid point everywhere: no other magnitude is closer to |W| * 2^-e
        scaled = torch.ldexp(w.double().abs(), -ek)
        best = (scaled[..., None] - GRID.double()).abs().amin(-1)
        assert torch.equal((scaled - _decode(q & 7).double()).abs(), best)
        # idempotent in value: quantising W' again gives the same weight
        assert torch.equal(quantize_blocks_e2m1(w_dq)[2].view(torch.int16), w_dq.view(torch.int16))
        assert torch.equal(quantize_blocks_e2m1(w.float())[2].view(torch.int16), w_dq.view(torch.int16))


def test_constructed_edges():
    from fo.quant import quantize_blocks_e2m1
    w = edge_weight_w4()
    q, e, w_dq = quantize_blocks_e2m1(w)
    assert e[3, 1] == 0 and not q[3, 32:64].any() and not w_dq[3, 32:64].any()
    # block maxima 6 * 2^-3 and 3 * 2^5 scale to exactly 6 (code 7); one ulp above 3 * 2^5 takes the next exponent
    assert e[4, 0] == -3 and q[4, 7] == 7
    assert e[4, 1] == 4 and q[4, 40] == 15 and w_dq[4, 40] == -96
    assert e[4, 2] == 5 and q[4, 70] == 5 and w_dq[4, 70] == 96
    # ties go to the even code, at both block exponents, for both signs
    for blk, ex in ((0, 0), (1, -4)):
        assert e[5, blk] == ex
        got = _decode(q[5, 32 * blk:32 * blk + 14])
        assert torch.equal(got, torch.cat([TIES_TO, -TIES_TO])), (blk, got)
        assert torch.equal(w_dq[5, 32 * blk:32 * blk + 14].float(), got * 2.0 ** ex)
        assert q[5, 32 * blk + 29] == 8 and q[5, 32 * blk + 30] == 0          # -0.1 -> -0, 0.1 -> +0
    assert q[5, 31] == 8 and torch.signbit(w_dq[5, 31].float())                # -0.0 keeps its sign
    # below the clamp: e = -125, 1.5 * 2^-126 -> 0.75 -> 1, -0.75 * 2^-126 -> 0.375 -> 0.5, 2^-130 -> 0, -2^-127 -> 0.25 -> 0
    assert e[6, 0] == -125
    assert q[6, :6].tolist() == [2, 9, 0, 8, 1, 8]
    assert w_dq[6, :6].float().tolist() == [2.0 ** -125, -2.0 ** -126, 0.0, -0.0, 2.0 ** -126, -0.0]


def test_packed_order():
    """Element by element against the layout text: codes [tile][ceil(K/128)][64 lanes][16 bytes], lane l of code step s
    holding row 16 tile + (l & 15), bytes 4 j .. 4 j + 3 its columns 128 s + 32 j + 8 (l >> 4) .. + 8, two per byte with
    the lower column in the low nibble; scale bytes e + 127 at [tile][ceil(K/128)][16 rows][4], byte j for k-step
    4 s + j; padding: zero codes, scale byte 127."""
    from fo.quant import pack_codes_w4, pack_scales_w4
    g = torch.Generator().manual_seed(4)
    for N, K in ((20, 96), (20, 160)):
        KK = (K + 127) // 128
        q = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
        e = torch.randint(-125, 120, (N, K // 32), generator=g, dtype=torch.int32)
        p = pack_codes_w4(q).view(2, KK, 64, 16)
        s = pack_scales_w4(e).view(2, KK, 16, 4)
        seen = torch.zeros(2, KK, 64, 16, 2, dtype=torch.bool)
        seen_s = torch.zeros(2, KK, 16, 4, dtype=torch.bool)
        for n in range(N):
            for k in range(K):
                t, st, j, lane = n // 16, k // 128, k % 128 // 32, 16 * (k % 32 // 8) + n % 16
                byte = int(p[t, st, lane, 4 * j + k % 8 // 2])
                assert (byte >> 4 if k % 2 else byte & 15) == int(q[n, k]), (n, k)
                seen[t, st, lane, 4 * j + k % 8 // 2, k % 2] = True
                assert int(s[t, st, n % 16, j]) == int(e[n, k // 32]) + 127, (n, k)
                seen_s[t, st, n % 16, j] = True
        lo, hi = p & 15, p >> 4
        assert not lo[~seen[..., 0]].any() and not hi[~seen[..., 1]].any()    # every other nibble: a zero code
        assert (s[~seen_s] == 127).all() and (~seen_s).any()                  # rows 20..31, k-steps past K
    assert (s[1, :, 4:] == 127).all() and (s[:, 1, :, 1:] == 127).all()       # (K = 160) rows 20..31, k-steps 5..7
    # the SwiGLU pair: gate tiles at even, up tiles at odd positions
    gu = pack_codes_w4(q, 1, 2, pack_codes_w4(q, 0, 2, torch.zeros(4 * 2048, dtype=torch.uint8))).view(4, 2048)
    assert torch.equal(gu[0], gu[1]) and torch.equal(gu[2], gu[3]) and torch.equal(gu[2], p[1].reshape(-1))
    sgu = pack_scales_w4(e, 1, 2, pack_scales_w4(e, 0, 2, torch.zeros(4 * 128, dtype=torch.uint8))).view(4, 128)
    assert torch.equal(sgu[0], sgu[1]) and torch.equal(sgu[3], s[1].reshape(-1))
    with pytest.raises(ValueError):
        from fo.quant import block_exponents
        block_exponents(torch.zeros(4, 100))


def _w4(lib, M=8, K=128, N=64, scale=FAKE, ntiles=None, swiglu=0):
    nt = (N + 15) // 16 * (2 if swiglu else 1) if ntiles is None else ntiles
    return lib.fo_gemm_w4(FAKE, K, M, K, FAKE, scale, nt, N, swiglu, FAKE, N, 0, None, 0, None, None, 0,
                          ctypes.c_float(0.0), None, None, None, None, None)


@needs_lib
def test_gemm_w4_refuses_before_touching_the_device():
    from fo import _lib
    lib, err = _lib.load(), _lib.last_error
    assert _w4(lib, M=17) == -2 and "M=17" in err(), err()
    assert _w4(lib, K=100) == -2 and "K=100" in err() and "multiple of 32" in err(), err()
    assert _w4(lib, scale=None) == -2 and "scale" in err(), err()
    assert _w4(lib, N=40, swiglu=1, ntiles=5) == -2 and "ntiles=5" in err() and "swiglu" in err(), err()
    assert _w4(lib, N=40, ntiles=2) == -2 and "ntiles=2" in err(), err()          # not the weight's tile count
    # a producer needs a plain launch
    assert lib.fo_gemm_w4(FAKE, 128, 8, 128, FAKE, FAKE, 8, 64, 1, FAKE, 64, 0, None, 0, None, None, 0,
                          ctypes.c_float(0.0), FAKE, FAKE, FAKE, None, None) == -2 and "sout" in err(), err()
    assert lib.fo_quant_w4(FAKE, 1, 16, 64, 32, FAKE, FAKE, None, 0, 1, None) == -2 and "ldw=32" in err(), err()
    assert lib.fo_quant_w4(FAKE, 1, 16, 100, 100, FAKE, FAKE, None, 0, 1, None) == -2 and "K=100" in err(), err()
    assert lib.fo_quant_w4_bytes(3584, 18944) == 224 * 148 * 1024
    assert lib.fo_quant_w4_bytes(20, 96) == 2048 and lib.fo_quant_w4_scale_bytes(20, 96) == 128


@needs_lib
def test_w4_counters_are_their_own():
    from fo import ops
    before = len(ops.LAUNCH_KINDS), ops._lib.load().fo_launch_counts(None, 0)
    assert ops._lib.load().fo_gemm_w4_counts(None, 0) == 3
    assert set(ops.w4_launch_counts()) == {"w4", "w4_xs", "w4_sk"}
    assert (len(ops.LAUNCH_KINDS), ops._lib.load().fo_launch_counts(None, 0)) == before == (25, 25)


def test_cli_accepts_mxfp4():
    import importlib
    inf, srv = importlib.import_module("bin.inference"), importlib.import_module("bin.server")
    base = ["--model_path", "m", "--llm_path", "l", "--input_wav", "i.wav", "--output_wav", "o.wav"]
    assert inf.get_args(base).llm_mlp_weights == "bf16"
    assert inf.get_args(base + ["--llm_mlp_weights", "mxfp4"]).llm_mlp_weights == "mxfp4"
    with pytest.raises(SystemExit):
        inf.get_args(base + ["--llm_mlp_weights", "int8"])
    assert srv.get_parser().parse_args([]).llm_mlp_weights is None      # the config's value, else bf16
    assert srv.get_parser().parse_args(["--llm_mlp_weights", "mxfp4"]).llm_mlp_weights == "mxfp4"
    with pytest.raises(SystemExit):
        srv.get_parser().parse_args(["--llm_mlp_weights", "int8"])


def test_fake_quant_source_takes_the_format():
    from fo.weights import FakeQuantSource
    assert FakeQuantSource(object()).fmt == "fp8" and FakeQuantSource(object(), "mxfp4").fmt == "mxfp4"
    with pytest.raises(ValueError):
        FakeQuantSource(object(), "int8")
