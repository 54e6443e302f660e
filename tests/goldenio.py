"""Goldens too large for one committed file (1 MiB a file) are stored as tests/golden/<stem>.partNN.npz.

save_parts() deals a fixture's arrays over compressed parts, each below the limit; an array too large for one part is
cut into flat pieces `name@i` beside its shape `name@shape`.  load_golden() gives back what np.load of the single
.npz gave: the same keys, dtypes, shapes and values, bit for bit.
"""
import glob
import io
import os

import numpy as np

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PIECE = 512 << 10     # raw bytes of one flat piece (its compressed size can only be about this or less)
LIMIT = 960 << 10     # compressed bytes of one part, under the 1 MiB limit with room for the zip directory


class Golden(dict):
    @property
    def files(self):
        return list(self)


def load_golden(name):
    """name: '<stem>.npz' under tests/golden, stored whole or in parts."""
    path = os.path.join(G, name)
    if os.path.exists(path):
        return np.load(path)
    parts = sorted(glob.glob(os.path.join(G, name[:-len(".npz")] + ".part??.npz")))
    if not parts:
        raise FileNotFoundError(path)
    out, pieces, shapes = Golden(), {}, {}
    for p in parts:
        with np.load(p) as z:
            for k in z.files:
                base, _, tag = k.partition("@")
                if not tag:
                    out[k] = z[k]
                elif tag == "shape":
                    shapes[base] = tuple(int(n) for n in z[k])
                else:
                    pieces.setdefault(base, {})[int(tag)] = z[k]
    for base, d in pieces.items():
        assert sorted(d) == list(range(len(d))), f"{name}: pieces of {base} missing"
        out[base] = np.concatenate([d[i] for i in range(len(d))]).reshape(shapes[base])
    return out


def _packed_size(k, v):
    b = io.BytesIO()
    np.savez_compressed(b, **{k: v})
    return b.tell()


def save_parts(name, arrays):
    """Write '<stem>.npz' (name) as <stem>.partNN.npz files under tests/golden; returns their paths."""
    stem = os.path.join(G, name[:-len(".npz")])
    for old in glob.glob(stem + ".part??.npz"):
        os.remove(old)
    items = []
    for k, v in arrays.items():
        v = np.asarray(v)
        assert "@" not in k
        if v.nbytes <= PIECE:
            items.append((k, v))
            continue
        flat, n = v.reshape(-1), max(1, PIECE // v.itemsize)
        items.append((k + "@shape", np.asarray(v.shape, dtype=np.int64)))
        items += [(f"{k}@{i}", flat[o:o + n]) for i, o in enumerate(range(0, flat.size, n))]
    parts, cur, size = [], {}, 0
    for k, v in items:
        s = _packed_size(k, v)
        if cur and size + s > LIMIT:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += s
    parts.append(cur)
    paths = []
    for i, p in enumerate(parts):
        paths.append(f"{stem}.part{i:02d}.npz")
        np.savez_compressed(paths[-1], **p)
        assert os.path.getsize(paths[-1]) < (1 << 20), paths[-1]
    return paths
