"""GPU: a data-parallel run saved by rank 0 and resumed by every rank
(tests/resume_dp_worker.py; two ranks on one GPU over gloo, started and
bounded as tests/test_gpu_dist.py starts its own).  Rank 0 alone writes the
file; both ranks load it and continue; afterwards the ranks' parameters and
Adam moments are equal to each other, and every rank's picks over the next
five steps are those of an uninterrupted two-rank run (the batch stream is a
function of (seed, global_step, rank), and the file carries the world size it
was written under)."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(worker, out, timeout=110, extra=()):
    port = _port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                   LOCAL_RANK=str(rank), WORLD_SIZE="2")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", worker),
                                       str(out), *extra], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=timeout)[0].decode(errors="replace"))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    assert all(p.returncode == 0 for p in procs), logs
    return json.loads(out.read_text())


def test_two_ranks_resume_from_rank_zeros_file(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    res = _run_ranks("resume_dp_worker.py", tmp_path / "resume.json",
                     extra=(str(tmp_path / "ckpt"),))
    print(res)
    assert res["world"] == 2 and res["world_in_file"] == [2, 2]
    # rank 0 alone wrote
    assert res["saved_here"] == [True, False] and res["files"] == ["state_epoch0001.pt"]
    assert res["loaded_step"] == [5, 5]
    assert res["n_params"] >= 10 and res["n_moments"] == 10
    assert res["params_equal"] and res["moments_equal"]
    assert res["n_picks"] == [5, 5] and res["picks_equal"] == [True, True]
    assert res["ranks_differ_in_picks"]
