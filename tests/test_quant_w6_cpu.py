"""The weight-only MXFP6 model on the host: the reference quantiser (fo.quant, the definition of mlp_weights="mxfp6"),
its accuracy beside the FP8 and MXFP4 quantisers, its packed order against the layout text of include/fo_hip.h, and
fo_gemm_w6 / fo_gemm_w6_head / fo_quant_w6's argument checks, which refuse before the library touches the device.  No
GPU needed."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("FO_LIB_PATH") or os.path.join(ROOT, "freeze-omni_amd", "fo", "libfo_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libfo_hip.so not built (run __graft_entry__.build())")

FAKE = 1 << 20   # dummy device addresses: never dereferenced by a refused call
# the e2m3 magnitudes, written out: subnormals, then three binades of 8
GRID = torch.tensor([0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0, 1.125, 1.25, 1.375, 1.5, 1.625, 1.75, 1.875,
                     2.0, 2.25, 2.5, 2.75, 3.0, 3.25, 3.5, 3.75, 4.0, 4.5, 5.0, 5.5, 6.0, 6.5, 7.0, 7.5])
# every midpoint between two neighbours, and the neighbour with the even code
TIES = (GRID[1:] + GRID[:-1]) / 2
TIES_TO = torch.stack([GRID[i + 1] if (i + 1) % 2 == 0 else GRID[i] for i in range(31)])


def edge_weight_w6():
    """20 x 96 (N no multiple of 16, K no multiple of 128), every value a bf16: random rows of mixed magnitude and
      row 3, block 1: all zero;
      row 4: block maxima exactly 7.5 * 2^-3, exactly 3.75 * 2^5 (mantissa 1.875: not above it) and the next bf16 above
             3.75 * 2^5;
      rows 5 and 7: every rounding tie at block exponent 0 (block 0, maximum 7.5) and at -4 (block 1), positive in row
             5 and negative in row 7; row 5, block 2 holds -0.0 and a -0.03 that rounds to zero with its sign kept;
      row 6, block 0: magnitudes below the clamp e >= -123 (maximum 1.5 * 2^-126 and fp32 denormals)."""
    g = torch.Generator().manual_seed(13)
    w = torch.randn(20, 96, generator=g) * torch.logspace(-8, 4, 20, base=2.0)[:, None]
    w[3, 32:64] = 0
    w[4] = w[4].clamp(-0.3, 0.3)
    w[4, 32:] *= 100
    w = w.to(torch.bfloat16).float()
    w[4, 7] = 7.5 * 2.0 ** -3
    w[4, 40] = -3.75 * 2.0 ** 5
    w[4, 70] = (3.75 + 2.0 ** -5) * 2.0 ** 5          # 1.875 * 2^6 plus one bf16 ulp
    ties = torch.cat([TIES, torch.tensor([7.5])])
    for row, sign in ((5, 1.0), (7, -1.0)):
        w[row, :32] = sign * ties
        w[row, 32:64] = sign * ties * 2.0 ** -4
    w[5, 64:96] = 0
    w[5, 64:68] = torch.tensor([7.5, -0.03125, 0.03125, -0.0])
    w[6, :32] = 0
    w[6, :6] = torch.tensor([1.5 * 2.0 ** -126, -0.75 * 2.0 ** -126, 2.0 ** -130, -2.0 ** -128, 2.0 ** -126, -2.0 ** -133])
    wb = w.to(torch.bfloat16)
    assert torch.equal(wb.float().view(torch.int32), w.view(torch.int32))       # bf16 values as written
    return wb


def _decode(q):
    mag = GRID[(q & 31).long()]
    return torch.where((q & 32) != 0, -mag, mag)


def test_grid_is_the_ocp_e2m3_grid():
    from fo.quant import E2M3_GRID
    assert torch.equal(torch.tensor(E2M3_GRID), GRID)
    for c in range(32):       # 2 exponent bits of bias 1, 3 mantissa bits
        ex, m = c >> 3, c & 7
        assert GRID[c] == (m / 8 if ex == 0 else (1 + m / 8) * 2.0 ** (ex - 1))


def test_reference_quantiser_properties():
    from fo.quant import block_exponents_e2m3, quantize_blocks_e2m3
    g = torch.Generator().manual_seed(2)
    for w in (edge_weight_w6(), torch.randn(48, 256, generator=g), (torch.rand(33, 64, generator=g) - 0.5) * 1e-3):
        N, K = w.shape
        q, e, w_dq = quantize_blocks_e2m3(w)
        assert q.dtype == torch.uint8 and q.shape == (N, K) and q.max() < 64
        assert e.dtype == torch.int32 and e.shape == (N, K // 32) and w_dq.dtype == torch.bfloat16
        assert torch.equal(e, block_exponents_e2m3(w))
        ek = e.repeat_interleave(32, dim=1)
        # W' = grid * 2^e exactly, and exactly a bf16 value
        exact = torch.ldexp(_decode(q).double(), ek)
        assert torch.equal(w_dq.double(), exact)
        assert torch.equal(w_dq.float().to(torch.bfloat16), w_dq)
        nz = w_dq != 0
        assert (w_dq[nz].float().abs() >= 2.0 ** -126).all()          # every non-zero W' is a normal bf16
        # the sign bit is the weight's, also where the magnitude rounded to zero
        assert torch.equal((q & 32) != 0, torch.signbit(w.float()))
        # scaled block maxima in (3.75, 7.5] (blocks above the clamp; an all-zero block has e = 0)
        amax = w.float().abs().view(N, K // 32, 32).amax(2)
        sm = torch.ldexp(amax.double(), -e)
        free = (amax > 0) & (e > -123)
        assert (sm[free] > 3.75).all() and (sm[free] <= 7.5).all()
        assert (e[amax == 0] == 0).all() and (e >= -123).all()
        assert (sm[(amax > 0) & (e == -123)] <= 7.5).all()
        # the nearest grid point everywhere: no other magnitude is closer to |W| * 2^-e
        scaled = torch.ldexp(w.double().abs(), -ek)
        best = (scaled[..., None] - GRID.double()).abs().amin(-1)
        assert torch.equal((scaled - _decode(q & 31).double()).abs(), best)
        # idempotent in value: quantising W' again gives the same weight
        assert torch.equal(quantize_blocks_e2m3(w_dq)[2].view(torch.int16), w_dq.view(torch.int16))
        assert torch.equal(quantize_blocks_e2m3(w.float())[2].view(torch.int16), w_dq.view(torch.int16))


def test_constructed_edges():
    from fo.quant import quantize_blocks_e2m3
    w = edge_weight_w6()
    q, e, w_dq = quantize_blocks_e2m3(w)
    assert e[3, 1] == 0 and not q[3, 32:64].any() and not w_dq[3, 32:64].any()
    # block maxima 7.5 * 2^-3 and 3.75 * 2^5 scale to exactly 7.5 (code 31); one ulp above takes the next exponent
    assert e[4, 0] == -3 and q[4, 7] == 31
    assert e[4, 1] == 4 and q[4, 40] == 63 and w_dq[4, 40] == -120
    assert e[4, 2] == 5 and q[4, 70] == 23 and w_dq[4, 70] == 120       # 121 / 32 = 3.78 -> 3.75
    # ties go to the even code, at both block exponents, for both signs
    assert TIES[0] == 0.0625 and TIES_TO[0] == 0 and TIES[1] == 0.1875 and TIES_TO[1] == 0.25
    assert TIES[30] == 7.25 and TIES_TO[30] == 7.0
    for row, sign in ((5, 1.0), (7, -1.0)):
        for blk, ex in ((0, 0), (1, -4)):
            assert e[row, blk] == ex
            got = _decode(q[row, 32 * blk:32 * blk + 31])
            assert torch.equal(got, sign * TIES_TO), (row, blk, got)
            assert torch.equal(w_dq[row, 32 * blk:32 * blk + 31].float(), got * 2.0 ** ex)
    assert q[5, 64:68].tolist() == [31, 32, 0, 32]                       # -0.03 -> -0, 0.03 -> +0, -0.0 keeps its sign
    assert torch.signbit(w_dq[5, 67].float()) and torch.signbit(w_dq[5, 65].float())
    # below the clamp: e = -123; 1.5 * 2^-126 -> 0.1875 -> 0.25 (tie, even code 2), -0.75 * 2^-126 -> 0.09375 -> 0.125,
    # 2^-130 -> 2^-7 -> 0, -2^-128 -> 2^-5 -> 0, 2^-126 -> 0.125, -2^-133 -> 0
    assert e[6, 0] == -123
    assert q[6, :6].tolist() == [2, 33, 0, 32, 1, 32]
    assert w_dq[6, :6].float().tolist() == [2.0 ** -125, -2.0 ** -126, 0.0, -0.0, 2.0 ** -126, -0.0]


def test_accuracy_sits_at_fp8_and_far_below_mxfp4():
    """Relative weight error on the seeded 512 x 3584 N(0, 1) / sqrt(K) weight: below 1.15 x the FP8 quantiser's and
    below 0.30 x the MXFP4 quantiser's, both arms computed here."""
    from fo.quant import quantize_blocks_e2m1, quantize_blocks_e2m3, quantize_rows_e4m3
    g = torch.Generator().manual_seed(0)
    w = torch.randn(512, 3584, generator=g) / 3584 ** 0.5
    err = lambda dq: float((dq.double() - w.double()).norm() / w.double().norm())
    e6, e8, e4 = err(quantize_blocks_e2m3(w)[2]), err(quantize_rows_e4m3(w)[2]), err(quantize_blocks_e2m1(w)[2])
    print(f"relative weight error: mxfp6 {e6:.4f} fp8 {e8:.4f} mxfp4 {e4:.4f}  ratios {e6 / e8:.3f} {e6 / e4:.3f}")
    assert e6 < 1.15 * e8
    assert e6 < 0.30 * e4


def _code_at(p, st, lane, j):
    """Code j of lane `lane` of code step st of one packed tile p [KK][2][64][12]: bits [6 j, 6 j + 6) of the lane's 24
    bytes (plane 0 then plane 1), little-endian."""
    field = bytes(p[st, 0, lane].tolist()) + bytes(p[st, 1, lane].tolist())
    return (int.from_bytes(field, "little") >> (6 * j)) & 63


def test_packed_order():
    """Element by element against the layout text: codes [tile][ceil(K/128)][2 planes][64 lanes][12 bytes], lane
    16 g + r of code step s holding columns 128 s + 32 g .. + 31 of row 16 tile + r, column j at bits [6 j, 6 j + 6) of
    the lane's 192-bit field whose dwords 0..2 are plane 0 and 3..5 plane 1; scale bytes e + 127 at
    [tile][ceil(K/128)][16 rows][4], byte g for lane group g; padding: zero codes, scale byte 127."""
    from fo.quant import pack_codes_w6, pack_scales_w6
    g = torch.Generator().manual_seed(4)
    for N, K in ((20, 96), (20, 160), (20, 192), (16, 128)):      # K % 128 = 96, 32, 64, 0; a ragged N
        nt, KK = (N + 15) // 16, (K + 127) // 128
        q = torch.randint(0, 64, (N, K), generator=g, dtype=torch.uint8)
        e = torch.randint(-123, 120, (N, K // 32), generator=g, dtype=torch.int32)
        p = pack_codes_w6(q).view(nt, KK, 2, 64, 12)
        s = pack_scales_w6(e).view(nt, KK, 16, 4)
        for t in range(nt):
            for st in range(KK):
                for lane in range(64):
                    r, gg = lane & 15, lane >> 4
                    n, k0 = 16 * t + r, 128 * st + 32 * gg
                    live = n < N and k0 < K
                    for j in range(32):
                        assert _code_at(p[t], st, lane, j) == (int(q[n, k0 + j]) if live else 0), (n, k0, j)
                    assert int(s[t, st, r, gg]) == (int(e[n, k0 // 32]) + 127 if live else 127), (n, k0)
    # the SwiGLU pair, tile_base / tile_stride = (0, 2) and (1, 2): gate tiles at even, up tiles at odd positions
    N, K = 20, 160
    q = torch.randint(0, 64, (N, K), generator=g, dtype=torch.uint8)
    q2 = torch.randint(0, 64, (N, K), generator=g, dtype=torch.uint8)
    e = torch.randint(-123, 120, (N, K // 32), generator=g, dtype=torch.int32)
    one, two = pack_codes_w6(q).view(2, -1), pack_codes_w6(q2).view(2, -1)
    gu = pack_codes_w6(q2, 1, 2, pack_codes_w6(q, 0, 2, torch.zeros(4 * 2 * 1536, dtype=torch.uint8))).view(4, -1)
    assert torch.equal(gu[0], one[0]) and torch.equal(gu[2], one[1])
    assert torch.equal(gu[1], two[0]) and torch.equal(gu[3], two[1])
    alone = pack_codes_w6(q, 1, 2).view(4, -1)                     # allocated for this weight: the other tiles zero
    assert not alone[0].any() and not alone[2].any() and torch.equal(alone[1], one[0]) and torch.equal(alone[3], one[1])
    s1 = pack_scales_w6(e).view(2, -1)
    sgu = pack_scales_w6(e, 1, 2, pack_scales_w6(e, 0, 2, torch.zeros(4 * 128, dtype=torch.uint8))).view(4, -1)
    assert torch.equal(sgu[0], sgu[1]) and torch.equal(sgu[3], s1[1]) and torch.equal(sgu[0], s1[0])
    salone = pack_scales_w6(e, 1, 2).view(4, -1)
    assert (salone[0] == 127).all() and torch.equal(salone[3], s1[1])
    with pytest.raises(ValueError):
        from fo.quant import block_exponents_e2m3
        block_exponents_e2m3(torch.zeros(4, 100))


def _w6(lib, M=8, K=128, N=64, X=FAKE, Q=FAKE, Y=FAKE, scale=FAKE, ntiles=None, swiglu=0):
    nt = (N + 15) // 16 * (2 if swiglu else 1) if ntiles is None else ntiles
    return lib.fo_gemm_w6(X, K, M, K, Q, scale, nt, N, swiglu, Y, N, 0, None, 0, None, None, 0,
                          ctypes.c_float(0.0), None, None, None, None, None)


def _w6h(lib, M=8, K=3584, N=64, X=FAKE, Q=FAKE, Y=FAKE, scale=FAKE, ntiles=None):
    return lib.fo_gemm_w6_head(X, K, M, K, Q, scale, (N + 15) // 16 if ntiles is None else ntiles, N, Y, N, None)


@needs_lib
def test_gemm_w6_refuses_before_touching_the_device():
    from fo import _lib, ops
    lib, err = _lib.load(), _lib.last_error
    ops.w6_launch_counts_reset()
    for call, name in ((_w6, "fo_gemm_w6:"), (_w6h, "fo_gemm_w6_head:")):
        assert call(lib, M=17) == -2 and "M=17" in err() and name in err(), err()
        assert call(lib, M=0) == -2 and "M=0" in err() and name in err(), err()
        assert call(lib, K=100) == -2 and "K=100" in err() and "multiple of 32" in err(), err()
        assert call(lib, X=None) == -2 and "NULL" in err() and name in err(), err()
        assert call(lib, Q=None) == -2 and "NULL" in err(), err()
        assert call(lib, Y=None) == -2 and "NULL" in err(), err()
        assert call(lib, scale=None) == -2 and "scale" in err(), err()
        assert call(lib, N=40, ntiles=2) == -2 and "ntiles=2" in err(), err()      # not the weight's tile count
    assert _w6(lib, N=40, swiglu=1, ntiles=5) == -2 and "ntiles=5" in err() and "swiglu" in err(), err()
    # codes of 2 GiB or more: 1,400,000 tiles x 1 code step x 1536 bytes (MXFP4's 1 KiB steps would still fit)
    assert _w6(lib, N=16 * 1400000) == -2 and "2 GiB" in err(), err()
    assert _w6h(lib, K=128) == -2 and "K=128" in err() and "3584" in err(), err()
    # a producer needs a plain launch
    assert lib.fo_gemm_w6(FAKE, 128, 8, 128, FAKE, FAKE, 8, 64, 1, FAKE, 64, 0, None, 0, None, None, 0,
                          ctypes.c_float(0.0), FAKE, FAKE, FAKE, None, None) == -2 and "sout" in err(), err()
    assert lib.fo_quant_w6(FAKE, 1, 16, 64, 32, FAKE, FAKE, None, 0, 1, None) == -2 and "ldw=32" in err(), err()
    assert lib.fo_quant_w6(FAKE, 1, 16, 100, 100, FAKE, FAKE, None, 0, 1, None) == -2 and "K=100" in err(), err()
    assert lib.fo_quant_w6(None, 1, 16, 64, 64, FAKE, FAKE, None, 0, 1, None) == -2 and "NULL" in err(), err()
    assert lib.fo_quant_w6(FAKE, 1, 16, 64, 64, FAKE, FAKE, None, -1, 1, None) == -2 and "tile_base" in err(), err()
    assert lib.fo_quant_w6_bytes(3584, 18944) == 224 * 148 * 1536
    assert lib.fo_quant_w6_bytes(20, 96) == 2 * 1536 and lib.fo_quant_w6_scale_bytes(20, 96) == 128
    assert not any(ops.w6_launch_counts().values())                 # a refused call is not counted


@needs_lib
def test_w6_counters_are_their_own():
    from fo import ops
    lib = ops._lib.load()
    before = len(ops.LAUNCH_KINDS), lib.fo_launch_counts(None, 0)
    assert lib.fo_gemm_w6_counts(None, 0) == 4
    assert tuple(ops.w6_launch_counts()) == ("w6", "w6_xs", "w6_sk", "w6_head")
    # the existing counters keep their shape
    assert lib.fo_gemm_w4_counts(None, 0) == 3 and lib.fo_gemm_head_counts(None, 0) == 2
    assert set(ops.w4_launch_counts()) == {"w4", "w4_xs", "w4_sk"}
    assert (len(ops.LAUNCH_KINDS), lib.fo_launch_counts(None, 0)) == before == (25, 25)


@needs_lib
def test_header_declares_the_entries():
    from fo import _lib
    txt = open(os.path.join(ROOT, "include", "fo_hip.h")).read()
    for name in ("fo_quant_w6_bytes", "fo_quant_w6_scale_bytes", "fo_quant_w6", "fo_gemm_w6", "fo_gemm_w6_head",
                 "fo_gemm_w6_counts", "fo_gemm_w6_counts_reset"):
        assert name + "(" in txt and name in _lib._SIGS and hasattr(_lib.load(), name), name


def test_cli_accepts_mxfp6():
    import importlib
    inf, srv = importlib.import_module("bin.inference"), importlib.import_module("bin.server")
    base = ["--model_path", "m", "--llm_path", "l", "--input_wav", "i.wav", "--output_wav", "o.wav"]
    for flag in ("llm_mlp_weights", "llm_lm_head_weights"):
        assert getattr(inf.get_args(base), flag) == "bf16"
        assert getattr(inf.get_args(base + ["--" + flag, "mxfp6"]), flag) == "mxfp6"
        assert getattr(srv.get_parser().parse_args([]), flag) is None      # the config's value, else bf16
        assert getattr(srv.get_parser().parse_args(["--" + flag, "mxfp6"]), flag) == "mxfp6"
    with pytest.raises(SystemExit):
        inf.get_args(base + ["--llm_attn_weights", "mxfp6"])                # the attention projections are not built
    with pytest.raises(SystemExit):
        srv.get_parser().parse_args(["--llm_attn_weights", "mxfp6"])


def test_fake_quant_source_takes_the_format():
    from fo.weights import FakeQuantSource
    s = FakeQuantSource(object(), "mxfp6", lm_head="mxfp6")
    assert s.fmt == "mxfp6" and s.lm_head == "mxfp6" and s.attn is None
    assert FakeQuantSource(object(), None, lm_head="mxfp6").fmt is None
    assert FakeQuantSource(object()).fmt == "fp8" and FakeQuantSource(object(), "mxfp4").fmt == "mxfp4"
    with pytest.raises(ValueError):
        FakeQuantSource(object(), "mxfp6", attn="mxfp6")
    with pytest.raises(ValueError):
        FakeQuantSource(object(), "mxfp8")


def test_engine_option_checks(monkeypatch):
    """The option checks come before anything touches a device or a model directory."""
    from fo.engine import FreezeOmniEngine
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    with pytest.raises(ValueError, match="mlp_fp8_rows=64 needs mlp_weights='fp8'"):
        FreezeOmniEngine("nowhere", mlp_weights="mxfp6", mlp_fp8_rows=64)
    with pytest.raises(ValueError, match="mlp_mxfp4_rows=64 needs mlp_weights='mxfp4'"):
        FreezeOmniEngine("nowhere", mlp_weights="mxfp6", mlp_mxfp4_rows=64)
    with pytest.raises(ValueError, match="attn_weights must be 'bf16', 'fp8' or 'mxfp4', got 'mxfp6'"):
        FreezeOmniEngine("nowhere", mlp_weights="mxfp6", lm_head_weights="mxfp6", attn_weights="mxfp6")
    with pytest.raises(ValueError, match="mlp_weights must be"):
        FreezeOmniEngine("nowhere", mlp_weights="mxfp8")
    with pytest.raises(ValueError, match="lm_head_weights must be"):
        FreezeOmniEngine("nowhere", lm_head_weights="mxfp8")
    # a legal combination passes the checks and goes on to look for the model
    with pytest.raises(Exception) as ei:
        FreezeOmniEngine("nowhere", mlp_weights="mxfp6", lm_head_weights="mxfp6", attn_weights="fp8", llm_kv="bf16")
    assert "must be" not in str(ei.value) and "needs mlp_weights" not in str(ei.value)
