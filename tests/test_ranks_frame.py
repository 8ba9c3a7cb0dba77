"""The launcher of the rank tests (tests/_ranks.py) on fake workers: small scripts in tmp_path that only print, sleep or exit.  No GPU
and no library call; the real worlds are tests/test_parallel_gloo.py (CPU) and the multi-rank GPU tests."""
import os
import subprocess
import sys
import time

import pytest

import _ranks
from _ranks import run_process_ranks

HERE = os.path.dirname(os.path.abspath(__file__))
GRACE = 2.0     # passed to the launcher in place of its 10 s, so that the bounds below stay short


@pytest.fixture
def popens(monkeypatch):
    """every Popen the launcher makes"""
    made = []

    class Recorded(subprocess.Popen):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    monkeypatch.setattr(_ranks.subprocess, "Popen", Recorded)
    return made


def _worker(tmp_path, body):
    path = tmp_path / "worker.py"
    path.write_text("import sys, time\nrank = int(sys.argv[1])\n" + body)
    return str(path)


def test_outputs_in_rank_order(tmp_path, popens):
    outs = run_process_ranks(_worker(tmp_path, "print(f'rank {rank} ok', sys.argv[2])\n"), 4, ["tag"])
    assert outs == [f"rank {r} ok tag\n" for r in range(4)]
    assert [p.returncode for p in popens] == [0] * 4


def test_a_failed_rank_ends_its_world(tmp_path, popens):
    """rank 1 exits with status 3 at once, the others would sleep for a minute: the launcher ends them.  The bound is the grace, which a
    child that ignored SIGTERM would use up, plus 5 s for starting four interpreters and one poll"""
    worker = _worker(tmp_path, "if rank == 1:\n    print('rank 1 gives up')\n    sys.exit(3)\ntime.sleep(60)\n")
    t0 = time.monotonic()
    with pytest.raises(AssertionError) as e:
        run_process_ranks(worker, 4, [], grace=GRACE)
    assert time.monotonic() - t0 < GRACE + 5
    msg = str(e.value)
    assert msg.startswith("rank 1 exited with status 3 first:"), msg
    assert "rank 1 gives up" in msg
    for r in (0, 2, 3):
        assert f"---- rank {r} (ended by the launcher" in msg, msg
    assert len(popens) == 4
    assert all(p.returncode is not None for p in popens)
    assert popens[1].returncode == 3
    assert all(popens[r].returncode < 0 for r in (0, 2, 3)), [p.returncode for p in popens]   # ended by a signal


def test_a_talkative_rank_cannot_block(tmp_path):
    """2 MB from rank 3 while rank 0 is still busy: more than a pipe holds, so a launcher that read rank by rank would leave rank 3
    stuck in its print"""
    worker = _worker(tmp_path, "if rank == 3:\n    sys.stdout.write('x' * (2 << 20) + '\\n')\nif rank == 0:\n    time.sleep(2)\n"
                               "print(f'rank {rank} ok')\n")
    outs = run_process_ranks(worker, 4, [], timeout=60)
    assert outs[3] == "x" * (2 << 20) + "\nrank 3 ok\n"
    assert outs[:3] == [f"rank {r} ok\n" for r in range(3)]


def test_the_deadline_ends_every_rank(tmp_path, popens):
    worker = _worker(tmp_path, "print(f'rank {rank} waits', flush=True)\ntime.sleep(60)\n")
    t0 = time.monotonic()
    with pytest.raises(AssertionError) as e:
        run_process_ranks(worker, 3, [], timeout=2, grace=GRACE)
    assert time.monotonic() - t0 < 2 + GRACE + 5
    msg = str(e.value)
    assert msg.startswith("deadline:") and "after 2 s" in msg, msg
    assert all(f"rank {r} waits" in msg for r in range(3)), msg
    assert len(popens) == 3 and all(p.returncode is not None and p.returncode < 0 for p in popens)


def test_commands_side_by_side(tmp_path):
    """the second entry point: its own environment per command, stdout and stderr apart"""
    path = tmp_path / "cmd.py"
    path.write_text("import os, sys\nprint(os.environ['WHICH'])\nprint('err', os.environ['WHICH'], file=sys.stderr)\n")
    res = _ranks.run_commands([([sys.executable, str(path)], dict(os.environ, WHICH=w)) for w in ("a", "b")], timeout=60)
    assert [(r.returncode, r.stdout, r.stderr) for r in res] == [(0, "a\n", "err a\n"), (0, "b\n", "err b\n")]


THREADS = """import sys
sys.path.insert(0, %r)
from _ranks import run_threads
calls = []


def finish(results):
    calls.append(results)
    print("finish", len(calls), results)


def body(rank, tw):
    if sys.argv[1] == "boom":
        if rank == 2:
            raise ValueError("boom")
        tw.barrier.wait(60)
    return "x=1"


run_threads(4, body, finish)
"""


def _threads(tmp_path, mode):
    path = tmp_path / "threads.py"
    path.write_text(THREADS % HERE)
    t0 = time.monotonic()
    out = subprocess.run([sys.executable, str(path), mode], capture_output=True, text=True, timeout=120)
    return out, time.monotonic() - t0


def test_run_threads_one_rank_raises(tmp_path):
    """the others wait at the barrier for up to 60 s; the abort lets them out through BrokenBarrierError at once"""
    out, seconds = _threads(tmp_path, "boom")
    assert out.returncode == 1, out.stdout + out.stderr
    assert seconds < 20
    assert "rank 2 FAILED:" in out.stdout and "ValueError: boom" in out.stdout
    assert " ok" not in out.stdout and "finish" not in out.stdout, out.stdout
    assert all(f"rank {r} FAILED:" in out.stdout for r in range(4))


def test_run_threads_every_rank_succeeds(tmp_path):
    out, _ = _threads(tmp_path, "fine")
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.splitlines() == [f"rank {r} ok x=1" for r in range(4)] + ["finish 1 ['x=1', 'x=1', 'x=1', 'x=1']"]
