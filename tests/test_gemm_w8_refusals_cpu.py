"""The argument checks the three FP8 weight-stream GEMM entries share (fo_gemm_w8, fo_gemm_w8_rows,
fo_gemm_w8_rows128), through the C-ABI and without a GPU: every refusal here is made before the entry's first HIP
call, so the made-up, suitably aligned addresses are never dereferenced.  Each one returns -2, names its own entry,
and launches nothing."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("FO_LIB_PATH") or os.path.join(ROOT, "freeze-omni_amd", "fo", "libfo_hip.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libfo_hip.so not built (run __graft_entry__.build())")

# entry -> (first row count, last row count, the band as its refusal words it)
ENTRIES = {"fo_gemm_w8": (1, 16, "M <= 16"), "fo_gemm_w8_rows": (17, 64, "17 <= M <= 64"),
           "fo_gemm_w8_rows128": (65, 128, "65 <= M <= 128")}
X, Q, SCALE, Y, WS, COUNTERS, STATS, GAMMA, YG = (0x100000 * i for i in range(1, 10))


def _args(**kw):
    """A launchable plain call of 100 columns (7 tiles) at K = 96, with `kw` replacing arguments by name."""
    a = dict(X=X, ldx=96, M=0, K=96, Q=Q, scale=SCALE, ntiles=7, N=100, swiglu=0, Y=Y, ldy=100, residual=0, ws=WS,
             ws_floats=1 << 25, counters=COUNTERS, rstats=None, rgroups=0, eps=1e-6, sout=None, gnext=None, yg=None,
             sgroups=None, stream=None)
    assert not set(kw) - set(a)
    a.update(kw)
    return tuple(a.values())


SWIGLU = dict(swiglu=1, ntiles=14)
# (case, arguments replaced, the words of the refusal)
SHARED = [
    ("M=0", dict(M=0), "bad shape"),
    ("K%32", dict(K=80, ldx=80), "K=80 must be a multiple of 32"),
    ("null-X", dict(X=None), "NULL X, Q or Y"),
    ("null-Q", dict(Q=None), "NULL X, Q or Y"),
    ("null-Y", dict(Y=None), "NULL X, Q or Y"),
    ("null-scale", dict(scale=None), "NULL scale"),
    ("ldx<K", dict(ldx=64), "X needs ldx=64 >= K=96"),
    ("ldx%4", dict(ldx=98), "X needs ldx=98 >= K=96"),
    ("X-misaligned", dict(X=X + 4), "16-byte alignment"),
    ("ldy<N", dict(ldy=96), "ldy=96 < N=100"),
    ("ntiles", dict(ntiles=8), "ntiles=8 packed tiles for N=100 columns"),
    ("ntiles-swiglu", dict(swiglu=1, ntiles=12), "ntiles=12 packed tiles for N=100 SwiGLU columns"),
    ("rstats-no-rgroups", dict(rstats=STATS), "rstats without rgroups"),
    ("sout-swiglu", dict(SWIGLU, sout=STATS), "sout needs a non-SwiGLU launch"),
    ("yg-no-gnext", dict(sout=STATS, yg=YG), "yg needs gnext"),
    ("yg-no-sout", dict(yg=YG, gnext=GAMMA), "yg comes with sout"),
    ("swiglu-residual", dict(SWIGLU, residual=1), "swiglu with residual unsupported"),
    # 4096 tiles of 512 code steps: (4096 + 4) KiB x 512 is past 2^31 bytes
    ("codes-2GiB", dict(N=65536, ldy=65536, ntiles=4096, K=32768, ldx=32768), "codes exceed 2 GiB"),
]


def _refused(entry, args, words):
    from fo import _lib, ops
    before = ops.launch_counts()
    rc = getattr(_lib.load(), entry)(*args)
    msg = _lib.last_error()
    assert rc == -2, (rc, msg)
    assert msg.startswith(entry + ": ") and words in msg, msg
    assert ops.launch_counts() == before


@pytest.mark.parametrize("case", SHARED, ids=[c[0] for c in SHARED])
@pytest.mark.parametrize("entry", ENTRIES)
def test_shared_refusal(entry, case):
    lo, hi, _ = ENTRIES[entry]
    _refused(entry, _args(**{"M": (lo + hi) // 2, **case[1]}), case[2])


@pytest.mark.parametrize("entry", ENTRIES)
def test_row_band(entry):
    """One row below the band and one above it are refused with the band's own text (below fo_gemm_w8's band lies
    M = 0, a bad shape); both ends of the band pass this check and are refused by the next one they fail."""
    lo, hi, band = ENTRIES[entry]
    _refused(entry, _args(M=hi + 1), band)
    _refused(entry, _args(M=lo - 1), band if lo > 1 else "bad shape")
    for M in (lo, hi):
        _refused(entry, _args(M=M, ldy=96), "ldy=96 < N=100")
