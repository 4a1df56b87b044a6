"""Developer study: where do the QPs that need a second ADMM round stand in the dispatch order?  The pre-pass's score (csrc/mpcqp_order.h,
restated in numpy by tools/order_fit.py) next to the round-1 score it replaced: class sizes, two-round QPs among the first H ranks
(H = 2048 is the first fill of a launch of 4096), and the costliest QPs' classes and ranks.  Needs a GPU for the iteration counts."""
import os, sys
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import mpcqp
import order_fit
B = 4096
for seed in (20250809, 1, 2, 3, 4):
    b = mpcqp.synth.make_batch(B, 10, 0.03, seed, order_fit.ALLG, order_fit.MUS)
    T, old = order_fit.terms(b)
    new = order_fit.classes(order_fit.score(T, order_fit.IN_SOURCE))
    sol = mpcqp.MPCBatch(N=10, precision="mixed")
    dev = sol.upload(b)
    o = sol.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"]); torch.cuda.synchronize()
    it = o["iters"].cpu().numpy(); admm, ps = mpcqp.split_iters(it)[0], mpcqp.split_iters(it)[1]
    hard = admm > 100
    cost = admm * 1.1 + ps * 9.0                     # us in a full device (profiles/r30_order_predictor.txt)
    top = np.argsort(-cost)[:12]
    for name, cls in (("round-1 score", old), ("this score   ", new)):
        rank = np.empty(B, int); rank[np.argsort(-cls, kind="stable")] = np.arange(B)   # dearest class first, batch order inside a class
        line = f"seed {seed} {name}: class sizes {np.bincount(cls, minlength=16).tolist()}; two-round QPs: {int(hard.sum())}"
        for H in (256, 512, 1024, 2048):
            line += f" | top {H}: {int((hard & (rank < H)).sum())}"
        print(line, flush=True)
        print("   the 12 costliest: class", cls[top].tolist(), "rank", rank[top].tolist(), "iters", admm[top].tolist())
