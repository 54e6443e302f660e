"""What mlp_weights="fp8" (or, with the second argument, "mxfp4" or "mxfp6") costs against the unquantised model on the
full-depth flow of tests/test_full_depth_gpu.py (real geometry, 28 Qwen2 layers, the engine's counter-hash weights): the system prompt, question.wav's 13 chunks (the
reference's fbank features, tests/golden/fbank.npz) with the user chat prefix, the assistant prefix and greedy text
steps.  Prints the state-probability differences per chunk, the decision-row logit differences under teacher forcing
with the bf16 engine's ids (and how often the arg-max agrees, against the bf16 top-2 margin), and where the two
engines' own greedy texts part.  A measurement, not a test.
python scripts/mlp_fp8_accuracy.py [steps] [fp8|mxfp4|mxfp6|bf16|a,b,..] [heads] [attns] (GPU only).  A comma-separated
second argument (`fp8,mxfp6,mxfp4`) measures each MLP mode in turn against the one bf16 engine of the process; a head
`same` then stands for the head of the MLP mode's own format.  The optional third argument is a
comma-separated list of lm_head_weights formats (`fp8,mxfp4`): each is measured against the bf16 engine in the same
process, over the MLP mode of the second argument (`bf16`: the head alone is quantised).  The optional fourth is a
comma-separated list of attn_weights formats, each measured under every head of the third (`bf16 bf16 fp8,mxfp4`: the
attention projections alone are quantised)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "freeze-omni_amd"))
from fo.engine import FreezeOmniEngine  # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 32
FMT = sys.argv[2] if len(sys.argv) > 2 else "fp8"
HEADS = sys.argv[3].split(",") if len(sys.argv) > 3 else ["bf16"]
ATTNS = sys.argv[4].split(",") if len(sys.argv) > 4 else ["bf16"]
SYS_IDS = list(range(1, 16))
USER_PREFIX = [151645, 198, 151644, 872, 198]
ASSIST_PREFIX = [151645, 198, 151644, 77091, 198]
dev = torch.device("cuda:0")
feats = np.load(os.path.join(ROOT, "tests", "golden", "fbank.npz"))["A_feats"]


def flow(eng, forced=None):
    llm, enc, ada = eng.llm, eng.enc["user"], eng.ada["user"]
    kv = llm.new_seq()
    probs, logits, toks = [], [], []
    try:
        llm.forward(llm.embed(SYS_IDS, round_fp16=True), [(kv, len(SYS_IDS))])
        ec, ac, pe = enc.new_cache(), ada.new_cache(), 0
        for c in range(len(feats)):
            out, T, pes = enc.infer(torch.from_numpy(feats[c][None]).to(dev), [ec], [pe])
            pe = pes[0]
            emb, To = ada(out, T, [ac])
            x = emb[:To]
            if c == 0:
                x = torch.cat([llm.embed(USER_PREFIX), x])
            x = x.half().float()
            h, bm = llm.forward(x, [(kv, x.shape[0])])
            probs.append(llm.state_probs(h, [bm.last_rows_host[0]]).cpu().numpy()[0])
        x = llm.embed(ASSIST_PREFIX, round_fp16=True)
        h, bm = llm.forward(x, [(kv, x.shape[0])])
        for j in range(STEPS):
            lg = llm.logits(h, [bm.last_rows_host[-1]]).float().cpu().numpy()[0]
            logits.append(lg)
            toks.append(int(lg.argmax()))
            h, bm = llm.forward(llm.embed([toks[-1] if forced is None else forced[j]], round_fp16=True), [(kv, 1)])
    finally:
        kv.free()
    return np.stack(probs), np.stack(logits), toks


def engine(mode, head="bf16", attn="bf16"):
    return FreezeOmniEngine(os.path.join(ROOT, "configs", "real"), device=dev, max_sessions=2, mlp_weights=mode,
                            lm_head_weights=head, attn_weights=attn)


eng = engine("bf16")
p0, l0, t0 = flow(eng)
del eng
torch.cuda.empty_cache()
for FMT, head, attn in ((f, f if h == "same" else h, a) for f in FMT.split(",") for h in HEADS for a in ATTNS):
    eng = engine(FMT, head, attn)
    print(f"mlp_weights={FMT}{'' if head == 'bf16' else f' lm_head_weights={head}'}"
          f"{'' if attn == 'bf16' else f' attn_weights={attn}'} against bf16:")
    p1, l1, t1f = flow(eng, forced=t0)
    _, _, t1 = flow(eng)
    del eng
    torch.cuda.empty_cache()
    dp = np.abs(p1 - p0)
    print(f"state probs over {len(p0)} chunks: max |diff| {dp.max():.2e}, mean {dp.mean():.2e} "
          f"(bf16 state_1 range {p0[:, 1].min():.3f}..{p0[:, 1].max():.3f})")
    dl = np.abs(l1 - l0)
    s = np.sort(l0, axis=1)
    margin = s[:, -1] - s[:, -2]
    agree = [a == b for a, b in zip(t0, t1f)]
    print(f"decision-row logits over {STEPS} teacher-forced steps: max |diff| {dl.max():.3e}, rms {np.sqrt((dl ** 2).mean()):.3e} "
          f"(logit std {l0.std():.3f}); arg-max equal {sum(agree)}/{STEPS}; bf16 top-2 margin min {margin.min():.3e}, "
          f"at the disagreeing steps {[round(float(m), 4) for m, a in zip(margin, agree) if not a]}")
    first = next((i for i, (a, b) in enumerate(zip(t0, t1)) if a != b), STEPS)
    print(f"greedy text, each engine on its own ids: equal for the first {first} of {STEPS} tokens")
