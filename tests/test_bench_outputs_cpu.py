"""bench.py's --dump-outputs and --full plumbing, on CPU: the arrays a turn hands over are assembled in a fixed order
(sentence by sentence, whatever order the worker threads released them in), written as float32 / float64 .npy, and an
over-large set is cut to a sample that is the same from run to run."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_full_and_dump_are_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 3, 1)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_turn_arrays_order_and_dtypes(tmp_path):
    B, T, D = 2, 3, 4
    seg = {(k, i): [torch.full((2 + k + i,), 10.0 * k + i), torch.full((1,), 10.0 * k + i + 0.5)]
           for k in range(2) for i in range(B)}
    # released out of order across sentences and users, in order within one (sentence, user)
    order = [(1, 0), (0, 1), (1, 1), (0, 0)]
    out = {"text_ids": [[1, 2, 3], [4, 5, 6]], "hiddens": [torch.full((B, D), float(t)) for t in range(T)],
           "codec_ids": {(0, 0): [7, 8], (0, 1): [9, 10], (1, 0): [11], (1, 1): [12, 13]},
           "segments": [(k, i, s) for j in range(2) for k, i in order for s in seg[k, i][j:j + 1]]}
    arr = bench.turn_arrays(out)
    assert sorted(arr) == ["codec_ids", "pcm_user00", "pcm_user01", "text_hidden", "text_ids"]
    assert arr["text_ids"].tolist() == [[1, 2, 3], [4, 5, 6]]
    assert arr["text_hidden"].shape == (B, T, D) and arr["text_hidden"][1, 2].tolist() == [2.0] * D
    assert arr["codec_ids"].tolist() == [[[7, 8], [11, -1]], [[9, 10], [12, 13]]]
    for i in range(B):
        want = torch.cat([s for k in range(2) for s in seg[k, i]]).numpy()
        np.testing.assert_array_equal(arr[f"pcm_user{i:02d}"], want)
    bench.dump_outputs(str(tmp_path / "o"), arr)
    for k, v in arr.items():
        got = np.load(tmp_path / "o" / (k + ".npy"))
        assert got.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(got, v)
    assert np.load(tmp_path / "o" / "pcm_user00.npy").dtype == np.float32


def test_dump_outputs_caps_with_a_repeatable_sample(tmp_path):
    rng = np.random.default_rng(1)
    arrays = {"big": rng.standard_normal((300, 100)).astype(np.float32), "ids": np.arange(10)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, limit=40000)
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    np.testing.assert_array_equal(a, b)
    ids = np.load(tmp_path / "a" / "ids.npy")
    assert ids.dtype == np.float64 and ids.tolist() == list(range(10))
    assert a.nbytes + ids.nbytes <= 40000 and a.size == 5000
    assert set(a.tolist()) <= set(arrays["big"].reshape(-1).tolist())
