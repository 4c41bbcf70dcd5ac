"""bench.py --dump-outputs: the arrays of the last timed step, on the seeded inputs, against the C restatement."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_are_the_timed_steps_results(tmp_path):
    from khoice_amd import synth
    from oracle import c_oracle as CO
    species, genomes, length, k = 3, 2, 200_000, 31
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--species", str(species), "--genomes", str(genomes), "--length", str(length), "--k", str(k),
                        "--no-cpu-baseline", "--dump-outputs", str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["steps"] == 2
    assert sorted(os.listdir(out)) == ["across_hist.npy", "distinct_per_seq.npy", "within_hist.npy"]
    got = {name: np.load(out / f"{name}.npy") for name in ("within_hist", "across_hist", "distinct_per_seq")}
    assert all(a.dtype == np.float64 for a in got.values())
    items = synth.species_set(species, genomes, length)
    want = CO.exp1([t for _, _, t in items], [s - 1 for s, _, _ in items], k, cs=5000, hist_len=5001, nthreads=4)
    for name, a in got.items():
        assert a.shape == want[name].shape, name
        assert (a == want[name].astype(np.float64)).all(), name
