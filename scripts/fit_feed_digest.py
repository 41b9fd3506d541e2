#!/usr/bin/env python3
"""Feed-sequence digest of the DGP fit drivers, without a GPU: what fit_dgp_labeledonly / fit_dgp hand to sess.run, iteration by iteration.

The synthetic project of tests/_project.py is trained with the trainer, the session and the frame uploader replaced by recorders, so a run
is the drivers' host side alone: set-up, schedule, batches, prints and snapshot names.  Per case the output holds one SHA-256 per iteration
over the feed dict (placeholder name, dtype, shape and bytes of every entry, None included, in sorted order), the objective handed to
minimize, the snapshot files written and the captured stdout (temporary paths and timings blanked).  Two revisions of the drivers feed the
same batches in the same order exactly when their outputs are equal:

    python scripts/fit_feed_digest.py --out digest.json [--depth 0|2]

tests/test_fit_drivers_cpu.py uses the same recorders."""
import argparse
import contextlib
import hashlib
import io
import json
import os
import random
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

START = "snapshot-step0-final--0"
CASES = {
    "labeledonly": lambda F, proj: F.fit_dgp_labeledonly(START, proj, maxiters=6),
    "dgp": lambda F, proj: F.fit_dgp(START, proj, batch_size=4, maxiters=6, gm2=1, gm3=3, n_max_frames=30, ns=3, aug=False),
    "dgp_aug": lambda F, proj: F.fit_dgp(START, proj, batch_size=4, maxiters=6, gm2=1, gm3=3, n_max_frames=30, ns=3, aug=True),
}


def feed_digest(feed_dict):
    h = hashlib.sha256()
    for name, v in sorted((k.name, v) for k, v in feed_dict.items()):
        h.update(name.encode())
        if v is None:
            h.update(b"|None;")
            continue
        a = np.ascontiguousarray(v)
        h.update(("|%s|%s|" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
        h.update(b";")
    return h.hexdigest()


class FakeTrainer:
    device = "cpu"

    def get_weights(self):          # one small entry: the real ResNet-50 weights take over a minute to write as bundles
        return {"pose/part_pred/block4/biases": np.zeros(3, dtype=np.float32)}


class FakeUploader:
    """Stands in for the frame uploader: hands the host frames on unchanged and counts its calls."""
    calls = 0

    def __init__(self, device, slots=4):
        self.device = device

    def __call__(self, images):
        FakeUploader.calls += 1
        return images


class RecordingSession:
    """Stands in for TrainSession: one digest per run, zero losses back."""
    digests, objectives = [], []

    def __init__(self, trainer, graph):
        self.trainer, self.graph = trainer, graph

    def run(self, fetches, feed_dict):
        loss, train_op = fetches
        RecordingSession.digests.append(feed_digest(feed_dict))
        RecordingSession.objectives.append(train_op.objective.name)
        return [{k: 0.0 for k in loss}, None]


@contextlib.contextmanager
def recorders(depth):
    """fitdgp / session with the recorders in place and PREFETCH_DEPTH = depth; everything is put back on exit."""
    from deepgraphpose_amd.models import fitdgp, session
    new = {(fitdgp, "PREFETCH_DEPTH"): depth, (fitdgp, "_make_trainer"): lambda *a, **k: FakeTrainer(),
           (session, "TrainSession"): RecordingSession}
    if hasattr(fitdgp, "_make_uploader"):
        new[(fitdgp, "_make_uploader")] = lambda trainer: FakeUploader(trainer.device) if fitdgp.PREFETCH_DEPTH > 0 else None
    else:
        new[(fitdgp, "_FrameUploader")] = FakeUploader
    old = {k: getattr(*k) for k in new}
    for (mod, name), v in new.items():
        setattr(mod, name, v)
    RecordingSession.digests, RecordingSession.objectives, FakeUploader.calls = [], [], 0
    try:
        yield fitdgp
    finally:
        for (mod, name), v in old.items():
            setattr(mod, name, v)


def train_dir(proj):
    return os.path.join(proj, "dlc-models", "iteration-0", "DemoOct2-trainset95shuffle1", "train")


def bare_project(root):
    """tests/_project.py's project without its start snapshot: the fake trainer never loads it, and writing ResNet-50 as a bundle takes
    longer than everything else here together."""
    from _project import make_project
    from deepgraphpose_amd import weights_io
    save, weights_io.save_weights = weights_io.save_weights, lambda *a, **k: None
    try:
        return make_project(root)[0]
    finally:
        weights_io.save_weights = save


def run_case(name, tmp, depth=2, call=None):
    """One driver call on a fresh project under `tmp` -> its record.  `call(fitdgp, proj)` overrides the case's own call."""
    root = os.path.join(str(tmp), name)
    os.makedirs(root)
    proj = bare_project(root)
    before = set(os.listdir(train_dir(proj)))
    np.random.seed(0)
    random.seed(0)
    out = io.StringIO()
    with recorders(depth) as fitdgp, contextlib.redirect_stdout(out):
        ret = (call or CASES[name])(fitdgp, proj)
        rec = dict(returned=repr(ret), digests=list(RecordingSession.digests), objectives=sorted(set(RecordingSession.objectives)),
                   uploader_calls=FakeUploader.calls)
    files = sorted(set(os.listdir(train_dir(proj))) - before)
    text = out.getvalue().replace(root, "<tmp>")
    text = re.sub(r"(running time: +|TOTAL TIME ELAPSED: +)[-+.e0-9]+", r"\1<t>", text)
    rec.update(files=files, snapshots=sorted({f.split(".")[0] for f in files if f.startswith("snapshot-")}), stdout=text, proj=proj)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="fit_feed_digest.json")
    ap.add_argument("--depth", type=int, default=2, help="PREFETCH_DEPTH of the run (0: inline, no uploader)")
    args = ap.parse_args()
    result = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in CASES:
            rec = run_case(name, tmp, args.depth)
            del rec["proj"], rec["uploader_calls"]          # (the uploader is not called at depth 0: not part of the identity)
            result[name] = rec
            print("%-12s %d iterations, %s, snapshots %s" % (name, len(rec["digests"]), rec["objectives"], rec["snapshots"]))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out, hashlib.sha256(open(args.out, "rb").read()).hexdigest()[:16])


if __name__ == "__main__":
    main()
