"""The one place that starts ranks for the tests: process-per-rank worlds (run_process_ranks, gloo_rank), independent processes side by
side (run_commands), and the ranks of a world as threads of one process (prepare_thread_rank_process, thread_rank, run_threads).

What all of it is for: a rank that fails ends its world.  Nobody waits for it, and nothing more is started on the card the ranks share."""
import contextlib
import os
import socket
import subprocess
import sys
import tempfile
import threading
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TAIL = 3000     # characters of a process's output that a failure message carries
POLL = 0.2      # seconds between two looks at the processes of a world
GRACE = 10.0    # seconds between terminate() and kill()


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ---- processes ---------------------------------------------------------------------------------------------------------------------------
def _end(procs, grace):
    """terminate() what still runs, kill() it after the grace, wait() in every case: no child is left, running or unreaped"""
    for p in procs:
        if p.poll() is None:
            p.terminate()
    end = time.monotonic() + grace
    for p in procs:
        try:
            p.wait(max(0.0, end - time.monotonic()))
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()


def _run_world(cmds, what, timeout, grace, merge):
    """Start every (argv, env) of cmds and poll them against ONE deadline.  The first that exits with a non-zero status, or the deadline,
    ends every other one (_end).  Output goes to temporary files, which cannot fill as a pipe can.  Returns one CompletedProcess per
    command (merge: stderr in stdout), or raises an AssertionError that names the first failure and carries everybody's tail."""
    procs, files = [], []
    first = None        # the first one seen with a non-zero status
    late = False
    try:
        for argv, env in cmds:
            fo = tempfile.TemporaryFile()
            fe = subprocess.STDOUT if merge else tempfile.TemporaryFile()
            files.append((fo, fe))
            procs.append(subprocess.Popen(argv, env=env, stdout=fo, stderr=fe))
        deadline = time.monotonic() + timeout
        while True:
            codes = [p.poll() for p in procs]
            first = next((i for i, c in enumerate(codes) if c), None)
            late = first is None and None in codes and time.monotonic() >= deadline
            if first is not None or late or None not in codes:
                break
            time.sleep(POLL)
    finally:
        own = [p.poll() for p in procs]      # how each one ended by itself: None where the launcher has to end it
        _end(procs, grace)
    res = []
    for (argv, _), p, (fo, fe) in zip(cmds, procs, files):
        texts = []
        for f in (fo,) if merge else (fo, fe):
            f.seek(0)
            texts.append(f.read().decode(errors="replace"))
            f.close()
        res.append(subprocess.CompletedProcess(argv, p.returncode, texts[0], None if merge else texts[1]))
    if first is None and not late:
        return res

    def tail(r):
        return (r.stdout + (r.stderr or ""))[-TAIL:]
    if late:
        msg = [f"deadline: {what}s {[i for i, c in enumerate(own) if c is None]} still ran after {timeout} s and were ended by the launcher"]
    else:
        msg = [f"{what} {first} exited with status {own[first]} first:\n{tail(res[first])}"]
    for i, r in enumerate(res):
        if i != first:
            how = f"ended by the launcher, status {r.returncode}" if own[i] is None else f"exited with status {own[i]}"
            msg.append(f"---- {what} {i} ({how}) ----\n{tail(r)}")
    raise AssertionError("\n".join(msg))


def run_process_ranks(worker, world, args, timeout=150, env=None, grace=GRACE):
    """One process per rank: [python, worker, rank, *args] for rank 0 .. world - 1, all against one deadline.  Returns every rank's stdout
    and stderr as one text, in rank order, after checking that each ended with status 0 and printed "rank r ok"."""
    cmds = [([sys.executable, worker, str(r)] + [str(a) for a in args], env) for r in range(world)]
    outs = [r.stdout for r in _run_world(cmds, "rank", timeout, grace, merge=True)]
    for r, out in enumerate(outs):
        print(f"---- rank {r} ----\n{out[-2500:]}")
    for r, out in enumerate(outs):
        assert f"rank {r} ok" in out, f"rank {r}:\n{out[-TAIL:]}"
    return outs


def run_commands(cmds, timeout=120, grace=GRACE):
    """Independent processes side by side, no ranks: cmds is a list of (argv, env).  The same polling and reaping as a world of ranks;
    returns one CompletedProcess per command, with stdout and stderr apart."""
    return _run_world(list(cmds), "command", timeout, grace, merge=False)


@contextlib.contextmanager
def gloo_rank(rank, world, port, cuda=True):
    """One rank of a gloo world, for a process worker.  A clean exit meets the others at a barrier and leaves the group; an exception does
    neither: the process dies with its traceback, and the launcher, which sees that at once, ends the others."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ["OMP_NUM_THREADS"] = "1"  # every worker runs the whole emulated-MPI oracle: no OpenMP teams fighting for the cores
    import torch
    import torch.distributed as dist
    if cuda:
        torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    yield
    dist.barrier()
    dist.destroy_process_group()


# ---- threads -----------------------------------------------------------------------------------------------------------------------------
def prepare_thread_rank_process(world):
    """What the process of a thread-rank world does before anything else touches HIP."""
    os.environ["OMP_NUM_THREADS"] = "8"
    # One hardware queue per rank.  The HIP runtime multiplexes the streams of a process onto GPU_MAX_HW_QUEUES hardware queues
    # (default 4): two ranks whose streams share a queue are serialised, and a halo kernel that waits for its neighbour's push would sit
    # in front of the very kernel that pushes.  (Process-per-rank runs have a queue set each.)  Must be set before HIP initialises, and set
    # outright: a smaller value inherited from the environment (HIP's default is 4) deadlocks the 4x2 and 2x2 grids.
    os.environ["GPU_MAX_HW_QUEUES"] = str(min(32, max(8, 3 * world)))  # each rank drives two streams (the exchange runs beside the interior sweep)
    import faulthandler
    faulthandler.dump_traceback_later(int(os.environ.get("MGX_TEST_WATCHDOG", "100")), exit=True)  # a stuck collective: all stacks, then exit
    import torch
    torch.cuda.set_device(0)


@contextlib.contextmanager
def thread_rank(tw, rank, p2p):
    """One rank of a thread world: its own HIP stream, its own libmgx.so instance (include/mgx.h: mgx_instance_*) and the ThreadComm that
    the body gets.  A clean exit waits for the others, cleans and destroys the instance.  An exception makes no further library or GPU
    call, no clean and no destroy: run_threads aborts the barrier, and the process ends."""
    import torch
    from mgroms_amd import nhydro, nhydro_clean
    from mgroms_amd._lib import check, lib
    from mgroms_amd.parallel import ThreadComm
    torch.cuda.set_device(0)
    torch.cuda.set_stream(torch.cuda.Stream())
    L = lib()
    inst = L.mgx_instance_create()
    check(L.mgx_instance_select(inst))
    assert L.mgx_instance_current() == inst
    nhydro.set_verbose(0)
    yield ThreadComm(tw, rank, p2p=p2p)
    tw.barrier.wait(120)
    nhydro_clean()
    check(L.mgx_instance_select(0))
    check(L.mgx_instance_destroy(inst))


def run_threads(world, body, finish=None):
    """The ranks of a world as daemon threads of this process, each running body(rank, tw) on one ThreadWorld.  A rank that raises aborts
    the barrier, so that nobody waits for it, and its traceback is kept.  Prints one line per rank, "rank r ok <what body returned>" or
    "rank r FAILED:" with the traceback; calls finish(results) when every rank succeeded; ends the process: status 1 if one did not."""
    from mgroms_amd.parallel import ThreadWorld
    tw = ThreadWorld(world)
    ok, results = [None] * world, [None] * world

    def run(rank):
        try:
            results[rank] = body(rank, tw)
            ok[rank] = True
        except BaseException:
            results[rank] = traceback.format_exc()
            ok[rank] = False
            try:
                tw.barrier.abort()
            except Exception:
                pass

    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    end = time.monotonic() + 90
    for t in th:
        t.join(max(0.0, end - time.monotonic()))
    ok = list(ok)
    for r in range(world):
        print(f"rank {r} did not finish" if ok[r] is None else f"rank {r} ok {results[r]}" if ok[r] else f"rank {r} FAILED:\n{results[r]}")
    if all(ok) and finish is not None:
        finish(results)
    sys.stdout.flush()
    os._exit(0 if all(ok) else 1)  # daemon threads may still sit in a collective after a failure
