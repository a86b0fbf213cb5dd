#!/usr/bin/env python3
"""Flagship benchmark: 4 KiB random-read IOPS + p99 latency on the
HBM-resident Malloc bdev, provisioned through the CSI control plane
(BASELINE.json metric: "4KiB randread IOPS + p99 lat, Malloc bdev via
CSI"), fio-shaped synthetic I/O at QD=32 per queue.

One rank per GPU (torch.distributed over RCCL when launched via
torch.distributed.run); each rank runs the full per-card stack —
hipstored daemon on its GPU + registry + controller + CSI driver — and
provisions its bdev via CSI CreateVolume -> registry proxy ->
controller -> hipstored, then attaches it with MapVolume (the
reference's signature flow). A *step* is a fixed batch of STEP_IOS
random 4 KiB reads per GPU measured in-daemon on persistent queues;
rank 0 prints one JSON line with the whole-job aggregate (weak scaling).

A plain run sets up, warms up, times K steps and prints the result
line; that is everything the benchmark measures, so --full (reserved
for secondary measurements) currently adds nothing.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W]
                       [--dump-outputs DIR] [--full]
"""

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

# Persistent service kernels need one real HW queue each (ROCm default
# is 4; beyond that MES time-slices them). Must precede HIP init.
# Assigned, not defaulted: hosts that export the runtime's own default
# of 4 would otherwise time-slice the 14 service kernels (measured
# 30k IOPS instead of 12M). HIPSTORE_HW_QUEUES overrides.
os.environ["GPU_MAX_HW_QUEUES"] = os.environ.get("HIPSTORE_HW_QUEUES", "24")


def _set_affinity_base(num_queues: int) -> None:
    """Pin each rank's daemon queue threads to a disjoint core range
    (SPDK-reactor style; spinning submitters jitter under CFS)."""
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    ncpu = os.cpu_count() or 1
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # Only pin when there are enough cores for every rank's queues.
    # Disjoint ranges per rank: perf-session queues first, then the
    # vhost slave's ring workers, then the native master's pollers
    # (spinning threads migrate under CFS — measured 3.4x on the vhost
    # path, tools/vhost_scale_probe.py).
    span = num_queues + 2
    if ncpu >= world * span:
        os.environ.setdefault("HIPSTORE_AFFINITY_BASE",
                              str(local_rank * span))
    if ncpu >= world * (span + 16):
        base = world * span + local_rank * 16
        os.environ.setdefault("HIPSTORE_VHOST_AFFINITY_BASE", str(base))
        os.environ.setdefault("HIPSTORE_MASTER_AFFINITY_BASE",
                              str(base + 8))

REPO_ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO_ROOT)

STEP_IOS = 131072  # 4 KiB reads per GPU per step (512 MiB moved)

# --dump-outputs: the timed path hands its caller counters only (the
# read payloads land in daemon-side pinned buffers), so the dump holds
# the last timed step's I/O count plus a fixed, seeded sample of the
# volume: DUMP_SAMPLE_IOS units are written with a seeded pattern before
# warm-up and read back through the bdev's vhost attachment after the
# timed steps — the bytes the engine serves from HBM for those offsets.
DUMP_SAMPLE_IOS = 256
DUMP_SEED = 0x0D0D
DUMP_MAX_IO = 512 << 10  # one I/O must fit the sample master's buffers


class SampleIO:
    """Seeded write-then-readback of a sample of the benchmark volume
    through a short-lived vhost-user master (never concurrent with the
    timed region's own session)."""

    def __init__(self, vhost_sock, personality, bdev_info, io_size):
        import random

        import numpy as np

        if io_size > DUMP_MAX_IO:
            raise SystemExit(f"--dump-outputs supports --io-size up to "
                             f"{DUMP_MAX_IO}")
        self.vhost_sock = vhost_sock
        self.personality = personality
        self.block_size = bdev_info.block_size
        self.io_size = io_size
        units = bdev_info.size_bytes // io_size
        # float32 on disk is 4 bytes per sampled byte: stay under 48 MiB
        count = min(DUMP_SAMPLE_IOS, units, (48 << 20) // (4 * io_size))
        self.units = sorted(random.Random(DUMP_SEED).sample(
            range(units), count))
        self.pattern = np.random.default_rng(DUMP_SEED).integers(
            0, 256, size=(count, io_size), dtype=np.uint8)

    def _master(self):
        from oim_amd.bench.vhost_client import VhostUserMaster
        master = VhostUserMaster(
            self.vhost_sock, queue=0 if self.personality == "blk" else 2)
        master.negotiate()
        return master

    def seed(self):
        master = self._master()
        try:
            for unit, row in zip(self.units, self.pattern):
                offset = unit * self.io_size
                if self.personality == "blk":
                    status, _ = master.blk_write(offset // 512, row.tobytes())
                else:
                    status = master.write16(
                        0, offset // self.block_size, row.tobytes(),
                        self.block_size).status
                if status != 0:
                    raise RuntimeError(f"sample write failed at {offset}")
        finally:
            master.close()

    def read_back(self):
        import numpy as np

        rows = []
        master = self._master()
        try:
            for unit in self.units:
                offset = unit * self.io_size
                if self.personality == "blk":
                    status, data = master.blk_read(offset // 512,
                                                   self.io_size)
                else:
                    result = master.read16(
                        0, offset // self.block_size,
                        self.io_size // self.block_size, self.block_size)
                    status, data = result.status, result.data
                if status != 0:
                    raise RuntimeError(f"sample read failed at {offset}")
                rows.append(np.frombuffer(data, dtype=np.uint8))
        finally:
            master.close()
        return np.stack(rows)


def write_dump(directory, sample, last_step):
    """DIR/io_count.npy (float64) and DIR/readback.npy (float32, one row
    per sampled I/O unit; 4 MiB at the default --io-size)."""
    import numpy as np

    os.makedirs(directory, exist_ok=True)
    np.save(os.path.join(directory, "io_count.npy"),
            np.array([last_step["io_count"]], dtype=np.float64))
    np.save(os.path.join(directory, "readback.npy"),
            sample.read_back().astype(np.float32))


def start_stack(rank, local_rank, use_gpu, args, tmp):
    """Per-rank control plane + data daemon; returns (client, cleanup)."""
    import grpc

    from oim_amd import hipstore, spec
    from oim_amd.common.server import grpc_target
    from oim_amd.controller import Controller, ControllerServer
    from oim_amd.csidriver import OIMDriver, RemoteBackend
    from oim_amd.registry import MemRegistryDB, Registry, RegistryServer
    from oim_amd.spec import csi_v1 as csi
    from oim_amd.spec.rpc_csi import CSIControllerStub

    _set_affinity_base(args.num_queues)
    daemon_sock = os.path.join(tmp, "hipstored.sock")
    cmd = [os.path.join(REPO_ROOT, "bin", "hipstored"), "-S", daemon_sock,
           "-d", str(local_rank)]
    daemon_env = dict(os.environ)
    if args.engine == "persistent":
        cmd.append("-P")
    elif args.engine == "shared":
        # one service kernel per device multiplexing all rings
        cmd.append("-P")
        daemon_env["HIPSTORE_SHARED"] = "1"
    if not use_gpu:
        cmd.append("-C")
    daemon = subprocess.Popen(cmd, stderr=subprocess.DEVNULL, env=daemon_env)
    deadline = time.time() + 60
    while not os.path.exists(daemon_sock):
        if daemon.poll() is not None:
            raise RuntimeError("hipstored exited early")
        if time.time() > deadline:
            raise RuntimeError("hipstored did not start")
        time.sleep(0.05)

    registry = Registry(db=MemRegistryDB())
    reg_server = RegistryServer(f"unix://{tmp}/registry.sock", registry)
    reg_server.start()
    controller_id = f"gpu-{rank}"
    controller = Controller(
        controller_id=controller_id,
        hipstored_socket=daemon_sock,
        controller_address=f"unix://{tmp}/controller.sock",
        registry_address=reg_server.addr(),
        registry_delay=3600.0,
    )
    ctrl_server = ControllerServer(f"unix://{tmp}/controller.sock", controller)
    ctrl_server.start()
    controller.register()
    backend = RemoteBackend(
        registry_address=reg_server.addr(), controller_id=controller_id)
    driver = OIMDriver(
        driver_name="oim-malloc", node_id=f"bench-node-{rank}",
        endpoint=f"unix://{tmp}/csi.sock", backend=backend)
    driver.start()

    # CSI CreateVolume -> proxy -> controller -> hipstored (HBM bdev).
    volume = f"bench-{rank}"
    size = int(args.bdev_gb * (1 << 30))
    with grpc.insecure_channel(grpc_target(f"unix://{tmp}/csi.sock")) as ch:
        stub = CSIControllerStub(ch)
        request = csi.CreateVolumeRequest(name=volume)
        request.capacity_range.required_bytes = size
        cap = request.volume_capabilities.add()
        cap.mount.fs_type = "ext4"
        cap.access_mode.mode = csi.ACCESS_MODE_SINGLE_NODE_WRITER
        stub.CreateVolume(request, timeout=120)
    # MapVolume through the proxy: attach the bdev to a SCSI target of
    # this card's vhost controller (completes the reference's NodeStage
    # control path; --frontend vhost then drives that same controller's
    # virtqueues for the timed region). Skipped for the vhost-blk
    # frontend, which claims the bdev with its own blk controller.
    if not (args.frontend == "vhost" and args.personality == "blk"):
        with grpc.insecure_channel(grpc_target(reg_server.addr())) as ch:
            stub = spec.ControllerStub(ch)
            stub.MapVolume(
                spec.MapVolumeRequest(volume_id=volume,
                                      malloc=spec.MallocParams()),
                metadata=((spec.CONTROLLER_ID_KEY, controller_id),),
                timeout=60)

    # Bounded RPC timeout: the daemon-side perf step has its own
    # deadline (~90 s wedge cutoff), so a dead daemon surfaces as a
    # socket timeout here instead of an unbounded hang (round 1 burned
    # a 30-minute driver budget on exactly this invoke).
    client = hipstore.Client(daemon_sock, timeout=180)

    def cleanup():
        client.close()
        driver.stop()
        ctrl_server.stop()
        reg_server.stop()
        daemon.terminate()
        try:
            daemon.wait(timeout=10)
        except subprocess.TimeoutExpired:
            daemon.kill()

    return client, volume, daemon_sock, cleanup


def main() -> int:
    parser = argparse.ArgumentParser()
    parser.add_argument("--gpus", type=int, default=1)
    parser.add_argument("--steps", type=int, default=20)
    parser.add_argument("--warmup", type=int, default=5)
    parser.add_argument("--io-size", type=int, default=4096)
    parser.add_argument("--queue-depth", type=int, default=32)
    parser.add_argument("--num-queues", type=int, default=14)
    parser.add_argument("--bdev-gb", type=float, default=8.0)
    parser.add_argument("--workload", default="randread")
    parser.add_argument("--engine", default="persistent",
                        choices=["batched", "persistent", "shared"],
                        help="HBM I/O engine: batched kernel launches, "
                             "per-queue service kernels, or the shared "
                             "one-kernel-per-device service")
    parser.add_argument("--frontend", default="daemon",
                        choices=["daemon", "vhost"],
                        help="timed data path: in-daemon perf session on "
                             "the bdev queues (SPDK-bdevperf analog), or "
                             "through the vhost-user front-end so every "
                             "timed byte crosses the virtqueue/host "
                             "boundary")
    parser.add_argument("--personality", default="scsi",
                        choices=["scsi", "blk"],
                        help="vhost frontend personality")
    parser.add_argument("--vhost-numjobs", type=int, default=4,
                        help="request rings for --frontend vhost")
    parser.add_argument("--vhost-master", default="native",
                        choices=["native", "python"],
                        help="vhost frontend driver: the C++ master "
                             "(measures the daemon's ceiling) or the "
                             "Python conformance master")
    parser.add_argument("--dump-outputs", metavar="DIR", default=None,
                        help="after the timed steps write DIR/io_count.npy "
                             "(I/Os the last step completed) and "
                             "DIR/readback.npy (seeded sample of the volume "
                             "read back through its vhost attachment), "
                             "both from rank 0")
    parser.add_argument("--full", action="store_true",
                        help="also run the benchmark's secondary "
                             "measurements; it has none today, so this "
                             "is the plain run")
    args = parser.parse_args()
    if args.steps < 1:
        parser.error("--steps must be at least 1")

    import torch
    import torch.distributed as dist

    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    distributed = world_size > 1
    use_gpu = torch.cuda.is_available()

    if distributed:
        dist.init_process_group(backend="nccl" if use_gpu else "gloo")
    if use_gpu:
        torch.cuda.set_device(local_rank)
        from oim_amd import _hipstore as hs
        if not hs.gpu_available():
            raise RuntimeError(
                "torch sees a GPU but oim_amd._hipstore does not — "
                "native extension not loaded; rebuild with `make`")

    if not use_gpu:
        args.bdev_gb = min(args.bdev_gb, 1.0)

    # Every socket of the stack lives in this directory and AF_UNIX
    # paths stop at 107 chars: keep clear of a deep system temp dir.
    tmp_root = tempfile.gettempdir()
    if len(tmp_root) > 64:
        tmp_root = "/tmp"
    with tempfile.TemporaryDirectory(prefix="oim-bench-",
                                     dir=tmp_root) as tmp:
        client, volume, daemon_sock, cleanup = start_stack(
            rank, local_rank, use_gpu, args, tmp)
        try:
            session = None
            attachment = None
            vhost_session = None
            sample = None
            if args.frontend == "vhost":
                # Timed region crosses the virtqueue: an in-process
                # vhost-user master (synthetic guest) drives request
                # rings against the daemon's slave, so every timed
                # byte traverses descriptor → ring worker → engine →
                # HBM → used ring (the reference's signature flow,
                # vhost_scsi.c process_requestq).
                from oim_amd import hipstore as hipstore_mod

                if args.personality == "scsi":
                    ctrlr = "vhost.0"  # MapVolume attached the bdev here
                else:
                    ctrlr = f"vhost-bench-{rank}"
                    client.invoke("construct_vhost_blk_controller",
                                  {"ctrlr": ctrlr, "dev_name": volume})
                bdev_info = hipstore_mod.get_bdevs(client, volume)[0]
                vhost_sock = os.path.join(os.path.dirname(daemon_sock),
                                          ctrlr)
                if args.dump_outputs and rank == 0:
                    sample = SampleIO(vhost_sock, args.personality,
                                      bdev_info, args.io_size)
                    sample.seed()

                if args.vhost_master == "native":
                    # C++ master, ONE standing session: the handshake
                    # and the slave's hipHostRegister of guest memory
                    # happen before the timed region; each step drives
                    # n_ios through the standing rings. (The Python
                    # master tops out ~30k IOPS and would measure the
                    # interpreter, not the daemon.)
                    from oim_amd import _hipstore as hs_native
                    vhost_session = hs_native.VhostMasterSession(
                        vhost_sock, args.personality,
                        args.vhost_numjobs, args.queue_depth,
                        args.io_size, bdev_info.block_size,
                        bdev_info.size_bytes)

                    def run_step(n_ios):
                        r = vhost_session.run(n_ios, args.workload)
                        return {"io_count": r["io_count"],
                                "iops": r["iops"],
                                "lat_p99_us": r["lat_p99_us"]}

                    attachment = None
                else:
                    import threading

                    from oim_amd.bench.vhost_harness import VhostAttachment
                    attachment = VhostAttachment(
                        client, daemon_sock, volume, ctrlr,
                        args.personality, args.vhost_numjobs,
                        args.queue_depth, args.io_size, args.workload,
                        create=False)

                    def run_step(n_ios):
                        jobs = attachment.jobs
                        per = (n_ios + len(jobs) - 1) // len(jobs)
                        for j in jobs:
                            j.lat_us.clear()
                        threads = [threading.Thread(target=j.run_count,
                                                    args=(per,))
                                   for j in jobs]
                        t0 = time.perf_counter()
                        for t in threads:
                            t.start()
                        for t in threads:
                            t.join()
                        dt = time.perf_counter() - t0
                        lat = sorted(x for j in jobs for x in j.lat_us)
                        count = per * len(jobs)
                        p99 = lat[min(len(lat) - 1, int(len(lat) * 0.99))] \
                            if lat else 0.0
                        return {"io_count": count, "iops": count / dt,
                                "lat_p99_us": p99}
            else:
                if args.dump_outputs and rank == 0:
                    from oim_amd import hipstore as hipstore_mod

                    # MapVolume attached the bdev to vhost.0, target 0.
                    sample = SampleIO(
                        os.path.join(os.path.dirname(daemon_sock), "vhost.0"),
                        "scsi", hipstore_mod.get_bdevs(client, volume)[0],
                        args.io_size)
                    sample.seed()
                session = client.invoke("perf_session_start", {
                    "bdev_name": volume,
                    "workload": args.workload,
                    "io_size": args.io_size,
                    "queue_depth": args.queue_depth,
                    "num_queues": args.num_queues,
                })["session_id"]

                def run_step(n_ios):
                    return client.invoke("perf_session_step", {
                        "session_id": session, "total_ios": n_ios})

            def barrier():
                if distributed:
                    dist.barrier()
                if use_gpu:
                    torch.cuda.synchronize()

            for i in range(args.warmup):
                r = run_step(STEP_IOS)
                print(f"[bench r{rank}] warmup {i + 1}/{args.warmup}: "
                      f"{r['iops']:.0f} IOPS", file=sys.stderr, flush=True)

            barrier()
            t0 = time.perf_counter()
            p99s = []
            ios_done = 0
            for i in range(args.steps):
                r = run_step(STEP_IOS)
                ios_done += r["io_count"]
                p99s.append(r["lat_p99_us"])
                # Progress to stderr so a killed run still leaves a tail.
                print(f"[bench r{rank}] step {i + 1}/{args.steps}: "
                      f"{r['iops']:.0f} IOPS p99={r['lat_p99_us']:.0f}us",
                      file=sys.stderr, flush=True)
            barrier()
            elapsed = time.perf_counter() - t0
            if session is not None:
                client.invoke("perf_session_stop", {"session_id": session})
            if attachment is not None:
                attachment.close()
            if sample is not None:
                # Drop the standing native session (run_step shares this
                # variable) so the controller accepts the sample master.
                vhost_session = None
                write_dump(args.dump_outputs, sample, r)
        finally:
            cleanup()

    if distributed:
        stats = torch.tensor([elapsed, float(ios_done), max(p99s)],
                             dtype=torch.float64)
        if use_gpu:
            stats = stats.cuda()
        gathered = [torch.zeros_like(stats) for _ in range(world_size)]
        dist.all_gather(gathered, stats)
        elapsed = max(g[0].item() for g in gathered)
        total_ios = sum(g[1].item() for g in gathered)
        p99 = max(g[2].item() for g in gathered)
    else:
        total_ios = float(ios_done)
        p99 = max(p99s)

    value = total_ios / elapsed
    if rank == 0:
        out = {
            # Defaults name BASELINE.json's metric (4KiB_randread_IOPS);
            # overriding --workload/--io-size relabels rather than
            # misreporting a different measurement under that name.
            "metric": f"{args.io_size // 1024}KiB_{args.workload}_IOPS",
            "value": round(value, 1),
            "unit": "IOPS",
            # Honest GPU count: the ranks that actually ran (--gpus is
            # only a hint; torchrun's WORLD_SIZE is ground truth).
            "n_gpus": world_size,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed * 1000 / args.steps, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "uint8",
            "data": "synthetic",
            "config": {
                "model": "hbm-malloc-bdev-via-csi",
                "global_batch": args.queue_depth * args.num_queues,
                "seq_len": args.io_size,
                "parallelism": f"1-card-per-gpu-x{world_size if distributed else 1}",
                "workload": args.workload,
                "io_size": args.io_size,
                "queue_depth": args.queue_depth,
                "num_queues": args.num_queues,
                "bdev_gb": args.bdev_gb,
                "step_ios_per_gpu": STEP_IOS,
                "backend": "hbm" if use_gpu else "cpu",
                "engine": args.engine,
                "frontend": args.frontend if args.frontend == "daemon"
                else f"vhost-user-{args.personality}"
                     f"-x{args.vhost_numjobs}rings-{args.vhost_master}",
                "provisioning": "csi-createvolume+proxy-mapvolume",
                "p99_us": round(p99, 1),
            },
        }
        print(json.dumps(out))
    if distributed:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
