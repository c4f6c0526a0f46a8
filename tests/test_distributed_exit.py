"""A rank that returns from its script without distributed.finish() still leaves its gloo group before the interpreter shuts down
(the group's worker threads, taken into shutdown alive, ended a finished rank of tests/test_distributed.py with SIGABRT under load)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r'''
import atexit, sys
sys.path.insert(0, {root!r})
import torch.distributed as dist
from storm_amd import distributed as D
atexit.register(lambda: print("AT_EXIT initialised=%d" % dist.is_initialized(), flush=True))   # registered first: runs last
D.init(backend="gloo", single_rank_group=True)
print("IN_SCRIPT initialised=%d" % dist.is_initialized(), flush=True)
if {finish}:
    D.finish()
'''


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(tmp_path, finish):
    script = tmp_path / "rank.py"
    script.write_text(SCRIPT.format(root=ROOT, finish=finish))
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), OMP_NUM_THREADS="1")
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    return [ln for ln in out.stdout.splitlines() if "initialised=" in ln]


def test_a_rank_without_finish_leaves_its_gloo_group_at_exit(tmp_path):
    assert _run(tmp_path, False) == ["IN_SCRIPT initialised=1", "AT_EXIT initialised=0"]


def test_the_exit_hook_is_a_no_op_after_finish(tmp_path):
    assert _run(tmp_path, True) == ["IN_SCRIPT initialised=1", "AT_EXIT initialised=0"]
