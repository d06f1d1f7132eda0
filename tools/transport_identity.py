"""Bit identity of the sharded runs across two builds of the library (FOSHIP_LIB=... selects the build, as tools/ab_bench.sh does).

    python tools/transport_identity.py --list
    FOSHIP_LIB=.../libfoship_ab.so python tools/transport_identity.py --case sdp-DR-ipc --out parent1/sdp-DR-ipc.npz
    python tools/transport_identity.py --compare parent1 parent2 new

One case per call, so that the caller can put every multi-process run under its own time limit.  The runs are those of
tests/test_gpu_peer_mailbox.py (its workers and its two-rank runner, imported from there): two ranks on one GPU, cone-sharded over
both kinds of mailboxes, and row-sharded over the host callback and the peer buffers.  Every rank's iterates (z after twelve
iterations, z2 after the first, zt with CG at its floor), CG counts, alpha12 history and status sums go to the .npz; --compare
reports np.array_equal per array, the first directory against each of the others.
"""
import argparse
import multiprocessing as mp
import socket
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

# name -> (runner, arguments)
CASES = {}
for _t in ("ipc", "host"):
    CASES["sdp-DR-%s" % _t] = ("cones", ("sdp", "DR", _t, False))
    CASES["sdp-tiles-GAPA-%s" % _t] = ("cones", ("sdp-tiles", "GAPA", _t, False))
    CASES["mixed-FISTA-%s" % _t] = ("cones", ("mixed", "FISTA", _t, False))
    CASES["sdp-DR-%s-direct" % _t] = ("cones", ("sdp", "DR", _t, True))
CASES["rows-mixed-DR-host"] = ("rows", ("DR", "host", "mixed"))
CASES["rows-mixed-DR-peer"] = ("rows", ("DR", "peer", "mixed"))


def run_rows(algname, transport, pname, iters=10, world=2):
    """test_row_sharded_two_processes_host_exchange's processes, without its comparisons"""
    import test_gpu_peer_mailbox as t
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=t._worker_rows, args=(r, world, port, algname, iters, q, transport, pname)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    try:
        for _ in range(world):
            r, payload = q.get(timeout=300)
            assert not isinstance(payload, str), payload
            got[r] = payload
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0, p.exitcode
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    return got


def flatten(got):
    out = {}
    for r, d in sorted(got.items()):
        for k, v in d.items():
            if v is None:
                continue
            if isinstance(v, dict):                    # status sums: one array, keys in sorted order
                v = [v[kk] for kk in sorted(v)]
            out["rank%d_%s" % (r, k)] = np.asarray(v, dtype=np.float64)
    return out


def compare(dirs):
    base, bad = Path(dirs[0]), 0
    for other in map(Path, dirs[1:]):
        for f in sorted(base.glob("*.npz")):
            a, b = np.load(f), np.load(other / f.name)
            diff = [k for k in a.files if k not in b.files or not np.array_equal(a[k], b[k])]
            worst = max((float(np.max(np.abs(a[k] - b[k]))) for k in diff if k in b.files and a[k].shape == b[k].shape), default=0.0)
            print("%-28s %s vs %s: %d arrays, %s" % (f.stem, base.name, other.name, len(a.files),
                                                      "array_equal" if not diff else "DIFFER in %s (max |a - b| = %.3e)" % (diff, worst)))
            bad += bool(diff)
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--case")
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs="+")
    a = ap.parse_args()
    if a.list:
        print("\n".join(CASES))
        return 0
    if a.compare:
        return 1 if compare(a.compare) else 0
    kind, args = CASES[a.case]
    if kind == "cones":
        import test_gpu_peer_mailbox as t
        got = t._run(*args)
    else:
        got = run_rows(*args)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    np.savez(a.out, **flatten(got))
    print("%s: %d arrays -> %s" % (a.case, len(flatten(got)), a.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
