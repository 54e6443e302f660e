#!/usr/bin/env python3
"""One SHA-256 per flow over everything the captured listen paths produce (fo.engine.ListenGraph, ListenPipe,
EncoderGraph): every chunk's state probabilities, decision hidden rows and pe_index, the final KV lengths, and each
session's K / V rows of every layer for positions 0 .. length-1, gathered through kv.slot(pos).

The launch sequences are deterministic, so two trees whose host code queues the same launches on the same metadata
print identical files.  Tiny config, the features of tests/golden/fbank.npz, seeded by position only.

    python scripts/listen_digest.py > digest.txt      (GPU only; ends itself after LIMIT_S seconds)
"""
import hashlib
import os
import signal
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "freeze-omni_amd"))
from fo.engine import FreezeOmniEngine  # noqa: E402

LIMIT_S = 300
ROLE = "<|im_start|>system\nYou are a helpful assistant."
dev = torch.device("cuda:0")
FEATS = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "fbank.npz"))["A_feats"]).to(dev)  # [13, 19, 80]


class Flow:
    """The sessions of one flow (forked from one system role) and the running hash of what their chunks return."""

    def __init__(self, eng, idents, stride):
        self.eng, self.idents, self.stride = eng, idents, stride
        self.base = eng.system_role(ROLE)
        self.kvs = [self.base.fork() for _ in idents]
        self.state = [dict(enc_cache=None, ada_cache=None, pe_index=0) for _ in idents]
        self.h = hashlib.sha256()
        self.chunks = 0

    def items(self, c):
        return [dict(identity=d, status="ipu_sl" if c == 0 else "ipu_cl", feats=FEATS[(c + self.stride * u) % 13],
                     kv=self.kvs[u], **self.state[u]) for u, d in enumerate(self.idents)]

    def carry(self, res):
        for u, r in enumerate(res):
            self.state[u] = dict(enc_cache=r["enc_cache"], ada_cache=r["ada_cache"], pe_index=r["pe_index"])

    def record(self, res):
        """One chunk's result list."""
        for r in res:
            p = r["probs"]
            self.h.update(b"none" if p is None else np.asarray([p["state_1"], p["state_2"]], np.float64).tobytes())
            buf, row = r["hidden_row"]
            self.h.update(buf[row].cpu().numpy().tobytes())
            self.h.update(np.asarray([r["pe_index"]], np.int64).tobytes())
        self.chunks += 1

    def finish(self, name):
        pool = self.eng.llm.pool
        lens = [kv.length for kv in self.kvs]
        self.h.update(np.asarray(lens, np.int64).tobytes())
        torch.cuda.synchronize()
        for kv in self.kvs:
            slots = torch.tensor([kv.slot(p) for p in range(kv.length)], dtype=torch.long, device=dev)
            for t in (pool.k, pool.v):
                rows = t[:, slots // pool.PS, :, slots % pool.PS]          # [position, layer, kv head, hd]
                self.h.update(rows.contiguous().view(torch.uint8).cpu().numpy().tobytes())
        for kv in self.kvs + [self.base]:
            kv.free()
        print(f"{name} chunks={self.chunks} lengths={lens} {self.h.hexdigest()}", flush=True)


def listen_flow(eng, name, idents, n_chunks, stride=4):
    """Chunk by chunk through engine.listen(): one identity -> the captured step (chunk 0 with the chat prefix);
    two identities -> the eager tick, its steady-state encoder stages replayed from EncoderGraphs."""
    f = Flow(eng, idents, stride)
    for c in range(n_chunks):
        res = eng.listen(f.items(c))
        f.carry(res)
        f.record(res)
    f.finish(name)


def pipe_flow(eng, name, n, n_chunks, C=1, first_in_pipe=True, refuse=None, stride=5):
    """Chunk 0 through listen() or, after apply_chat_prefix, through the pipe like the rest; C chunks per Qwen2
    stage; refuse: decide() says no on that chunk's results, and a further push must raise."""
    f = Flow(eng, ["user"] * n, stride)
    pipe = eng.listen_pipe(C)
    asked = [0 if first_in_pipe else 1]   # the chunk whose results decide() sees next

    def decide(res):
        asked[0] += 1
        return asked[0] - 1 != refuse

    def record(out):
        for res in ([out] if C == 1 else out) if out is not None else []:
            f.record(res)

    for c in range(n_chunks):
        items = f.items(c)
        if c == 0 and not first_in_pipe:
            res = eng.listen(items)
            f.carry(res)
            f.record(res)
            continue
        if c == 0:
            items = eng.apply_chat_prefix(items)
            f.carry(items)
        pe_next, prev = pipe.push(items, decide if refuse is not None else None)
        for u in range(n):
            f.state[u]["pe_index"] = pe_next[u]
        record(prev)
        if pipe.stopped:
            try:
                pipe.push(items)
            except RuntimeError:
                break
            raise AssertionError("a push after the refusal did not raise")
    assert pipe.stopped == (refuse is not None)
    if not pipe.stopped:
        record(pipe.flush())
    f.finish(name)


def main():
    signal.alarm(LIMIT_S)   # no handler: the default action ends the process
    eng = FreezeOmniEngine(os.path.join(ROOT, "configs", "tiny"), device=dev, max_sessions=16)
    listen_flow(eng, "1 listen(graph) 3x7", ["user"] * 3, 7)
    pipe_flow(eng, "2a pipe 3x9 chunk 0 through listen()", 3, 9, first_in_pipe=False)
    pipe_flow(eng, "2b pipe 3x9 chunk 0 in the pipe", 3, 9)
    pipe_flow(eng, "3 pipe 2x8 refusal on chunk 4", 2, 8, first_in_pipe=False, refuse=4, stride=3)
    for C, n_chunks in ((2, 9), (3, 3), (4, 10), (7, 16), (8, 17)):
        pipe_flow(eng, f"4 pipe({C}) 3x{n_chunks}", 3, n_chunks, C=C)
    pipe_flow(eng, "5 pipe(3) 2x12 refusal on chunk 4", 2, 12, C=3, refuse=4, stride=3)
    listen_flow(eng, "6 eager two-identity listen 2+2 sessions, opening tick + 3", ["user", "system"] * 2, 4, stride=3)
    del eng
    eng = FreezeOmniEngine(os.path.join(ROOT, "configs", "tiny"), device=dev, max_sessions=16, llm_kv="bf16")
    pipe_flow(eng, "7 bf16 KV: pipe 3x9 chunk 0 through listen()", 3, 9, first_in_pipe=False)
    pipe_flow(eng, "7 bf16 KV: pipe 3x9 chunk 0 in the pipe", 3, 9)
    pipe_flow(eng, "7 bf16 KV: pipe(8) 3x17", 3, 17, C=8)


if __name__ == "__main__":
    main()
