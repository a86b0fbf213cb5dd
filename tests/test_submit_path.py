"""Host pieces of the submit path, without a GPU.

The sharded I/O statistics of Bdev must stay exact whichever thread
submits, and the RPC that reports them must look as it did. The
pinned-range registry and the shard arithmetic have a stand-alone C++
program of their own (tests/native/submit_path_test.cpp, `make
submit-path-test` also runs it under ThreadSanitizer); here it is built
plain and run once.
"""

import os
import subprocess

from oim_amd import hipstore

from fixtures import hipstored  # noqa: F401  (fixture)

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IO = 4096
QUEUES = 4


def run_session(client, bdev, workload, total_ios):
    started = client.invoke("perf_session_start", {
        "bdev_name": bdev, "workload": workload, "io_size": IO,
        "queue_depth": 8, "num_queues": QUEUES})
    try:
        step = client.invoke("perf_session_step", {
            "session_id": started["session_id"], "total_ios": total_ios})
    finally:
        client.invoke("perf_session_stop",
                      {"session_id": started["session_id"]})
    return step["io_count"]


def test_iostat_exact_from_four_queues(hipstored):  # noqa: F811
    """3 x 2000 reads, then 2 x 1000 writes, of 4 KiB from 4 queue
    threads each: get_bdevs_iostat reports exactly those, summed over
    the threads' shards, under the names it always had."""
    with hipstore.Client(hipstored.socket_path) as client:
        hipstore.construct_malloc_bdev(client, 16384, 512, name="exact0")
        reads = sum(run_session(client, "exact0", "randread", 2000)
                    for _ in range(3))
        writes = sum(run_session(client, "exact0", "randwrite", 1000)
                     for _ in range(2))
        assert (reads, writes) == (6000, 2000)
        entry = client.invoke("get_bdevs_iostat",
                              {"name": "exact0"})["bdevs"][0]
        assert entry == {
            "name": "exact0",
            "num_read_ops": reads,
            "num_write_ops": writes,
            "num_unmap_ops": 0,
            "bytes_read": reads * IO,
            "bytes_written": writes * IO,
        }
        typed = hipstore.get_bdevs_iostat(client, "exact0")[0]
        assert (typed.num_read_ops, typed.bytes_written) == (reads,
                                                             writes * IO)
        hipstore.delete_bdev(client, "exact0")


def test_iostat_binding_matches_sync_io():
    """Bdev.iostat() of the Python module: the synchronous helpers'
    requests, counted from this thread."""
    from oim_amd import _hipstore as hs

    bdev = hs.create_malloc_bdev("exact1", 512, 4096)
    assert bdev.iostat() == dict(num_read_ops=0, num_write_ops=0,
                                 num_unmap_ops=0, bytes_read=0,
                                 bytes_written=0)
    bdev.write(0, bytes(8192))
    bdev.write(8192, bytes(512))
    assert bdev.read(0, 4096) == bytes(4096)
    bdev.fill(4096, 7, 1024)
    assert bdev.iostat() == dict(num_read_ops=1, num_write_ops=2,
                                 num_unmap_ops=1, bytes_read=4096,
                                 bytes_written=8704)


def test_standalone_program():
    """The range registry's and the shards' own checks (hit, miss,
    removal, re-registration through a remembered entry, touching
    ranges, a tile across a range's end, eight readers against one
    writer; eight threads x 100 000 accounted requests)."""
    target = "native/build/submit_path_test"
    subprocess.run(["make", target], cwd=REPO_ROOT, check=True,
                   capture_output=True, timeout=300)
    proc = subprocess.run([os.path.join(REPO_ROOT, target)],
                          capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "submit_path_test: ok" in proc.stdout
