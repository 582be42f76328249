"""CPU side of the sharded local search: the gloo all-gather behind Screener.comm_init_host (pcramp_amd.shard.gloo_allgather)
and the new entry points of the C-ABI.  The GPU side is tests/test_gpu_sharded_search.py."""
import os
import socket
import sys

import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _worker(rank, world, port, tmp):
    import datetime
    import torch.distributed as dist
    from pcramp_amd import shard
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, world_size=world, rank=rank,
                            timeout=datetime.timedelta(seconds=120))
    try:
        ag = shard.gloo_allgather()
        got = ag(bytes([rank + 1]) * 5 + bytes([200 + rank]))
        with open(os.path.join(tmp, "r%d" % rank), "wb") as f:
            f.write(got)
    finally:
        dist.destroy_process_group()


def test_gloo_allgather_rank_order(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    world = 3
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    want = b"".join(bytes([r + 1]) * 5 + bytes([200 + r]) for r in range(world))
    for r in range(world):
        assert (tmp_path / ("r%d" % r)).read_bytes() == want


def test_shard_entry_points_exist():
    """pcr_comm_init_host / pcr_shard_targets / pcr_shard_combine_mode are part of the library; without a handle they refuse."""
    from pcramp_amd import api
    L = api.load_library()
    assert L.pcr_shard_combine_mode(None) == 0
    assert L.pcr_shard_targets(None, None, 0, 0) == -1
    cb = api.HOST_ALLGATHER(lambda s, n, r, u: 0)
    assert not L.pcr_comm_init_host(None, 2, 0, cb, None)
    assert L.pcr_comm_world(None) == 0
