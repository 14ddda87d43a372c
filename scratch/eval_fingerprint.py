"""Fingerprint of the eval plan for one precision mode, the sibling of plan_fingerprint.py: the golden state at B = 2,
128x224, printed as ONE JSON line with mc_query_workspace mode 0, the SHA-256 of the ten maps of forward_infer and the
SHA-256 of the outputs of backbone_forward -> neck_forward -> head_forward chained.  Two builds of the library that plan
the same launches print the same line, byte for byte.  With MONOCON_HIP_PROFILE_DUMP=1 the per-op "fprof" lines of the
plan (every op, its shape and its cfg) go to stderr.

    python scratch/eval_fingerprint.py f16x2
"""
import hashlib, json, os, sys
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "monocon-pytorch_amd"), REPO):
    sys.path.insert(0, p)
from hipmonocon import synth
from hipmonocon.engine import Engine

mode = sys.argv[1] if len(sys.argv) > 1 else "f16x2"
B, H, W = 2, 128, 224
stats = np.load(os.path.join(REPO, "tests", "golden", "bn_calib_seed7.npz"))


def digest(named):
    h = hashlib.sha256()
    for name, t in named:
        h.update(name.encode())
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


e = Engine()
e.set_precision({"fp32": 0, "bf16": 1, "bf16x3": 2, "f16x2": 3}[mode])
state = {k: v.to(e.device) for k, v in synth.make_state_dict(7, bn_stats={k: stats[k] for k in stats.files}).items()}
e.bind_state(state)
img = synth.make_batch(501, B, H, W, with_labels=False)["img"].to(e.device).contiguous()
query = e.query_workspace(B, H, W, "infer")
preds = e.forward_infer(img)
levels = e.backbone_forward(img)
staged = e.head_forward(e.neck_forward(levels))
if os.environ.get("MONOCON_HIP_PROFILE_DUMP"):
    e.forward_infer(img)
    e.profile_forward(1)
print(json.dumps({"mode": mode, "shape": [B, H, W], "query_workspace": query, "forward_infer": digest(sorted(preds.items())),
                  "stages": digest(sorted(staged.items()))}, sort_keys=True))
