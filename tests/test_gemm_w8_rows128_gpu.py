"""fo_gemm_w8_rows128 (the FP8 weight stream for 65..128 rows, PackedLinearW8(stream_rows=128)): the tests of
tests/test_gemm_w8_rows_gpu.py at band 128."""
import pytest

from test_gemm_w8_rows_gpu import band_tests

pytestmark = pytest.mark.gpu

globals().update(band_tests(128))
