"""fos_exchange_bench, two ranks on one GPU, one mailbox kind per call: python tools/exchange_ab.py ipc|host ROUNDS  (FOSHIP_LIB selects the build)."""
import multiprocessing as mp
import os
import socket
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def worker(rank, world, port, transport, rounds, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, str(ROOT))
    import torch.distributed as dist
    import __graft_entry__ as ge
    pkg = ge.load_package()
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        prob = pkg.workloads.c4_block_sdp(nblocks=8, k=16, p=6)
        lp = pkg.sharding.shard_problem(prob, world, rank).problem
        dev = pkg.HipHSDE(lp.A, lp.b, lp.c, lp.K1, lp.K2)
        if transport == "host":
            dev.peer_open_host(world, rank, "/foship-xb-%d" % port, timeout_s=10.0)
        else:
            handles = [None] * world
            dist.all_gather_object(handles, dev.peer_export())
            dev.peer_open(world, rank, handles, timeout_s=10.0)
        dist.barrier()
        assert dev.peer_selftest(16)
        dev.peer_enable(True)
        dist.barrier()
        us = dev.exchange_bench(rounds)
        q.put((rank, us))
        dist.barrier()
        dev.close()
        dist.destroy_process_group()
    except Exception as exc:  # noqa: BLE001
        q.put((rank, "error: " + repr(exc)))


def main():
    transport, rounds, world = sys.argv[1], int(sys.argv[2]), 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, world, port, transport, rounds, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    try:
        for _ in range(world):
            r, v = q.get(timeout=120)
            assert not isinstance(v, str), v
            got[r] = v
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0, p.exitcode
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    lib = os.path.basename(os.environ.get("FOSHIP_LIB", "libfoship.so"))
    print("exchange %s %s rounds=%d us_per_exchange rank0=%.4f rank1=%.4f" % (lib, transport, rounds, got[0], got[1]), flush=True)


if __name__ == "__main__":
    main()
