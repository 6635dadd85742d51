#!/usr/bin/env python
"""bench.py -- edges/s (and nodes/s) per message-passing layer on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload cfg3|cfg2] [--dump-outputs DIR] [--full]

`--gpus N` with N > 1 may be started either way: under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ...
bench.py --gpus N ...` (what the driver does; RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* come from the environment), or
plainly as `python bench.py --gpus N`, which re-executes itself under torch.distributed.run on 127.0.0.1 (the reference's
multi-GPU entry spawns its ranks from one process too: distributedtrainer.py:250-265).

One "step" = one pass of the hot path over one minibatch whose inputs are already resident in HBM: build the graph plan
(dst-sorted CSR) for that minibatch + every message-passing layer of the workload.  Nothing is cached across steps (the
plan cache is cleared each step).

Primary workload: the batch BASELINE.json quotes its metric on -- the Graph2Class-style batch of configs[2] (48 graphs,
~116k nodes, 8 raw -> 17 edge types, Typilus GGNN stack: 8 GGNN layers, hidden 128, max aggregation, fp32, forward).
`value` = E / t_layer (edges per second per message-passing layer, E counted after reverse + self augmentation) and
`ms_per_step` = the wall time of the K timed steps / K.

A plain run does only that: build the inputs, W warm-up steps, the K timed steps, the outputs of the last timed step
(`--dump-outputs DIR`: one DIR/<name>.npy per array the step returns, float32 / float64, a fixed seeded row sample of the
node tables when they exceed 64 MB together; rank 0's at N > 1), the JSON line.

`--full` adds everything else, after the timed steps: the per-kernel HIP-event pass (`kernels`, `roofline`), the
single-minibatch replay, `repeats`, the >= 10 s sustained block, and at N=1 the other configs, each with its own
full-size parity against the CPU oracle (benchmarks/*.py):
  config1            configs[0] as the reference batches it (3 000-node cap): GGNN-64 layer and the shipped PPI stack
  config2            configs[1]: synthetic 200k / 1.1M graph, one MLP-MP layer
  config3_sum        configs[2] with sum aggregation
  config4, config4_ggnn   configs[3] on one GPU: the shipped MLP-MP stack and the GGNN variant with global exchange
  config5_shard      the per-GPU shard of configs[4], every row checked; sharded_cfg5: the same shard through the dst-range
                     code path (process group, halo all-to-all) with its one-GPU counterpart beside it
  graph2class_train, readme_default_arch    training steps (the README's own quantity)
  cpu_baseline       the CPU restatement timed on this box's host cores
`parity` (top level) rolls every config up: `strict_1e-5` and `configs_on_relaxed_bar`.  A parity miss fails the run (exit
code 3).  The `--no-*` options drop single parts of a `--full` run.

N>1: the path partitions over whole graphs (a minibatch is a disjoint union; the reference's own multi-GPU mode hands
whole graphs to ranks), so every rank runs the single-GPU step on ITS OWN Graph2Class batch: no data-path collective,
weak scaling.  With `--full` the dst-range-sharded cut-edge workloads run after it (ptgnn_amd.sharded: halo all-to-all
over RCCL): `sharded_cfg5` (top level) and `cut_edges_variant`.

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import socket
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from benchmarks import common as C  # noqa: E402
from benchmarks.common import _log  # noqa: E402


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--workload", default="cfg3", choices=["cfg3", "cfg2"])
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write what the last timed step returned as DIR/<name>.npy (float32 / float64, <= 64 MB in all)")
    p.add_argument("--full", action="store_true",
                   help="after the timed steps also run the kernel pass, roofline, repeats, sustained block, secondary "
                        "configs, sharded variants, CPU baseline and oracle parity (a plain run does none of them)")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--gemm", default=None, choices=["tile", "stream"],
                   help="kernel family / arithmetic of the dense blocks for the PRIMARY line (default: stream = exact fp32)")
    p.add_argument("--no-secondary", action="store_true")
    p.add_argument("--no-rotation", action="store_true",
                   help="cfg3: replay ONE minibatch in the timed region (the rounds 1-4 form) instead of rotating over four")
    p.add_argument("--no-sustained", action="store_true", help="skip the >= 10 s sustained block of the primary step")
    p.add_argument("--sustained-seconds", type=float, default=10.0)
    p.add_argument("--force-sharded", action="store_true",
                   help="run the dst-range-sharded code path (process group, halo all-to-all) even at N=1")
    p.add_argument("--cut-edges", action="store_true",
                   help="N>1: ONE random graph over all ranks ((N-1)/N of the edges cut, halo all-to-all per "
                        "layer) instead of the default one-graph-per-rank partition")
    p.add_argument("--sharded-variants", action="store_true",
                   help="N>1: after the primary measurement also time the two ptgnn_amd.sharded variants "
                        "(global ids / cut edges) and report them as secondary entries")
    p.add_argument("--global-ids", action="store_true",
                   help="N>1: the per-rank graphs as ONE disjoint-union batch with global node ids, split by "
                        "ptgnn_amd.sharded (no-cut detection = one all-reduce per minibatch)")
    p.add_argument("--no-sharded-variants", action="store_true",
                   help="skip the dst-range-sharded cut-edge workloads (cfg5 shard; at N>1 also the cfg4 stack) that a "
                        "--full run times after the primary measurement")
    a = p.parse_args()
    if a.steps < 1:
        p.error("--steps must be >= 1")
    a.force_sharded = a.force_sharded or a.global_ids or a.cut_edges   # all three need the process group
    return a


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def self_launch(args) -> int:
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves, one per GPU over RCCL on 127.0.0.1
    (LOCAL_RANK -> device, bound in benchmarks.common.dist_setup).  Rank 0's single JSON line passes through this
    process's stdout; the exit code is the ranks'."""
    shared = os.environ.get("PTGNN_AMD_BENCH_SHARE_GPU", "0") not in ("", "0")
    have = torch.cuda.device_count()
    if have < args.gpus and not shared:
        raise SystemExit(f"--gpus {args.gpus}: this node shows {have} GPU(s) (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES?)")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC: RCCL across processes needs it on this stack
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // max(args.gpus, 1))))
    _log(f"no WORLD_SIZE in the environment: launching {args.gpus} ranks under torch.distributed.run")
    return subprocess.call(cmd, env=env)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU path)")
    C.hold_stdout()
    rank, world, dev = C.dist_setup(args)
    # N = 1, --full: the cfg5 shard also runs through the dst-range code path (world-1 process group, nothing cut) unless
    # skipped
    sharded_leg = ((args.full and not args.no_sharded_variants and not args.no_secondary) or args.sharded_variants
                   or args.force_sharded)
    from benchmarks import cpu_baseline as CPU, graph2class as G2C, synthetic as SYN
    # CPU legs before the final thread sweep (the cfg4 / cfg5 oracle parity) run on a bounded pool: a 256-thread
    # OpenMP pool on a quota-limited container oversubscribes, and its spinning workers then slow every later
    # host-side step of this process (measured: 29 s to build a batch that takes 1 s)
    torch.set_num_threads(max(1, min(16, CPU._thread_counts()[-1])))
    from ptgnn_amd import _lib, ops
    _lib.load()
    ops.set_gemm_mode(args.gemm or "stream")
    gemm_names = {0: "f32 (exact fp32 MFMA, 128x128 tile kernels)", 1: "f32 (exact fp32 MFMA, streaming kernels)"}

    rotation = None
    if args.workload == "cfg2":
        st = SYN.make_cfg2(dev, rank, world, args.force_sharded or args.global_ids, args.cut_edges)
        step = lambda: SYN.step_cfg2(st, world)  # noqa: E731
    else:
        # The timed K steps ROTATE over four minibatches of different seeds (round 5): replaying one minibatch keeps its
        # states, messages and weights warm in the 256 MiB Infinity Cache and flattered the round-4 headline by ~2 %
        # (3.84 vs 3.92 ms sustained).  Rank r draws minibatches r, r + world, r + 2 world, ...; parity and the CPU
        # baseline use the first one; the single-minibatch replay figure is reported beside the headline.
        rotation = [G2C.make_cfg3(dev, rank + world * i) for i in range(1 if args.no_rotation else G2C.ROTATE_MINIBATCHES)]
        st = rotation[0]
        turn = {"i": 0}

        def step():
            cur = rotation[turn["i"] % len(rotation)]
            turn["i"] += 1
            return G2C.step_cfg3(cur)

    _log(f"workload {args.workload} built; timing the primary region")
    launched = ops.launch_counts()        # host-side counters of the library: no device work, nothing timed
    seconds, last_out = C.timed_steps(step, args.steps, args.warmup, world, dev)
    launched = ops.launches_since(launched)
    ms_per_step = seconds / args.steps * 1e3
    _log(f"primary: {ms_per_step:.3f} ms/step")
    if args.dump_outputs and rank == 0:
        shapes = C.dump_outputs(args.dump_outputs, C.output_arrays(last_out))
        _log(f"outputs of the last timed step -> {args.dump_outputs}: {shapes}")
    del last_out
    summary = C.kernel_pass(step, args.steps, world) if args.full else None
    layers = st["layers_per_step"]
    if rotation is not None:   # mean over the K timed steps (step i of the run uses minibatch i mod 4; W warm-ups came first)
        timed = [rotation[(args.warmup + i) % len(rotation)] for i in range(args.steps)]
        e_mine, n_mine = sum(t["E"] for t in timed) / args.steps, sum(t["N"] for t in timed) / args.steps
    else:
        e_mine, n_mine = st["E"], st["N"]
    edges_all_ranks = C.sum_over_ranks(e_mine, world, dev)       # per-rank batches differ in size
    nodes_all_ranks = C.sum_over_ranks(n_mine, world, dev)
    value = edges_all_ranks / (seconds / args.steps / layers)

    result = {
        "metric": "edges/sec per MP layer", "value": round(value, 1), "unit": "edges/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32",
        "data": "synthetic", "gemm_mode": gemm_names[ops.get_gemm_mode()],
        "config": {"workload": st["desc"], "nodes_per_gpu": st["N"], "edges_per_gpu": st["E"],
                   "hidden": st["H"], "mp_layers_per_step": layers, "mode": "forward (inference), fp32",
                   "plan_build_in_step": True,
                   # GGNN edge form: one GEMM row per distinct (edge type, source) pair of the batch, read per edge by
                   # the aggregation -- the unit of `value` stays the edge (ptgnn_amd.ops.GraphPlan.unique_messages)
                   "message_rows": ("shared per (edge type, source) pair" if launched.get("k_stream_edge_shared")
                                    else "one per edge"),
                   "parallelism": ("single GPU" if world == 1 else
                                   f"{world} GPUs x whole graphs (one batch per GPU), no data-path collective")
                   if "adj" in st else (
                       f"dst-range shard x{world} + halo all-to-all per layer" if st.get("cut_edges") else
                       f"dst-range shard x{world} on graph boundaries (no cut edges => no data-path collective)")},
        "nodes_per_sec_per_layer": round(nodes_all_ranks / (seconds / args.steps / layers), 1),
        "edges_per_sec_readme_convention": round(edges_all_ranks / (seconds / args.steps), 1),
    }
    if summary is not None:
        ktab = C.kernel_table(summary)
        dominant = max(ktab, key=lambda k: ktab[k]["total_ms"])
        roof = {k: ktab[dominant][k] for k in ("bound", "achieved", "peak", "unit", "frac",
                                               "algorithmic_bytes_per_launch")}
        roof.update(kernel=dominant, avg_ms=ktab[dominant]["avg_ms"])
        roof.update(C.pmc_traffic(args.workload, dominant))
        result.update(roofline=roof, kernels=ktab)
    exit_code = 0
    parities = {}
    if rotation is not None and len(rotation) > 1:
        result["config"]["minibatches_rotated"] = len(rotation)
        # `value` = edges_per_gpu / (ms_per_step / layers): the MEAN over the timed steps (the per-minibatch sizes are listed below)
        result["config"]["edges_per_gpu"] = round(e_mine, 1)
        result["config"]["nodes_per_gpu"] = round(n_mine, 1)
        result["config"]["nodes_per_minibatch"] = [t["N"] for t in rotation]
        result["config"]["edges_per_minibatch"] = [t["E"] for t in rotation]
    if args.full and rotation is not None and len(rotation) > 1:
        try:      # the round-1..4 form of the headline (one minibatch replayed), beside the rotating one
            sec1, _ = C.timed_region(lambda: G2C.step_cfg3(st), args.steps, 2, world, dev)
            result["single_minibatch_replay"] = {
                "ms_per_step": round(sec1 / args.steps * 1e3, 4),
                "value": round(C.sum_over_ranks(st["E"], world, dev) / (sec1 / args.steps / layers), 1),
                "note": "one minibatch replayed K times (the rounds 1-4 headline form): its working set stays cache-warm"}
        except Exception as exc:  # noqa: BLE001
            result["single_minibatch_replay"] = {"error": f"{type(exc).__name__}: {exc}"}
    if args.workload == "cfg3":
        result["vs_readme_v100_inference_2527k"] = round(result["edges_per_sec_readme_convention"] / world / 2.527e6, 2)

    if world > 1 and args.workload == "cfg2" and "adj" in st and args.sharded_variants:
        # the same weak-scaling work through ptgnn_amd.sharded: (a) global ids, partition on graph boundaries
        # (one all-reduce per minibatch, no per-layer exchange); (b) cut edges: RCCL halo all-to-all per layer
        k2 = max(5, args.steps // 2)
        for key, cut in (("global_ids_variant", False), ("cut_edges_variant", True)):
            try:   # secondary numbers must never cost the primary line
                st2 = SYN.make_cfg2(dev, rank, world, True, cut)
                sec2, _ = C.timed_region(lambda: SYN.step_cfg2(st2, world), k2, 2, world, dev)
                result[key] = {"workload": st2["desc"], "ms_per_step": round(sec2 / k2 * 1e3, 4),
                               "edges_per_sec_per_layer": round(st2["E"] * world / (sec2 / k2), 1)}
                del st2
            except Exception as exc:  # noqa: BLE001
                result[key] = {"error": f"{type(exc).__name__}: {exc}"}
                break              # ranks may have diverged: do not enter another collective section
    def sharded_variants():
        from benchmarks import dst_range
        try:
            C.late_group(dev)
            dst_range.run_variants(result, rank, world, dev)
        except Exception as exc:  # noqa: BLE001  (world = 1 only: at N > 1 run_variants handles its own failures)
            result["sharded_cfg5"] = {"error": f"{type(exc).__name__}: {exc}"}
        if world == 1:
            # the collective backend's helper threads (RCCL watchdog / heartbeat) compete with this process's launch
            # loop for the host: a launch-bound secondary measured 7 % slower with the group alive (round 6)
            C.drop_group()

    if world > 1 and ((args.full and not args.no_sharded_variants) or args.sharded_variants):
        sharded_variants()
    if rank == 0 and world == 1 and not (args.force_sharded and args.workload == "cfg2"):
        if args.full:
            result["repeats"] = C.repeat_stats(step, args.steps)
        if args.full and args.workload == "cfg3" and not args.no_sustained:
            _log("sustained: >= 10 s of the primary step over 4 rotating minibatches")
            try:
                result["sustained"] = G2C.sustained_stats(dev, seconds=args.sustained_seconds)
            except Exception as exc:  # noqa: BLE001  (never costs the primary line)
                result["sustained"] = {"error": f"{type(exc).__name__}: {exc}"}
            torch.cuda.empty_cache()
        if args.full and not args.no_secondary:
            check = not args.no_cpu_baseline

            def leg(key, fn, parity_of=lambda r: r.get("parity")):
                """One secondary config: its numbers never cost the primary line; its parity record joins the rollup and
                a miss fails the run."""
                nonlocal exit_code
                _log(f"secondary: {key}")
                try:
                    result[key] = fn()
                    rec = parity_of(result[key])
                    if check and rec is not None:
                        parities[key] = rec
                        if not rec.get("ok", True):
                            exit_code = 3
                except Exception as exc:  # noqa: BLE001
                    result[key] = {"error": f"{type(exc).__name__}: {exc}"}
                torch.cuda.empty_cache()

            if args.workload == "cfg3":
                from benchmarks import ppi, varmisuse
                leg("config2", lambda: SYN.config2(dev, max(10, args.steps), parity=check))
                leg("config3_sum", lambda: G2C.config3_sum(dev, args.steps, parity=check))
                leg("config1", lambda: ppi.config1(dev, parity=check),
                    parity_of=lambda r: {k: r[k]["parity"] for k in ("ggnn64", "ppi_arch_mlp256") if "parity" in r[k]} or None)
                leg("config5_shard", lambda: SYN.config5_shard(dev, parity=check))
                leg("config4", lambda: varmisuse.config4(dev, parity=check))
                leg("config4_ggnn", lambda: varmisuse.config4(dev, parity=check, arch="ggnn"))
            else:
                leg("graph2class", lambda: G2C.graph2class_forward(dev, max(10, args.steps // 2)))
            _log("secondary: Graph2Class training steps")
            result["graph2class_train"] = [G2C.train_cfg3(dev, 0.0), G2C.train_cfg3(dev, 0.1)]
            torch.cuda.empty_cache()
            # like for like with README.md:15-18: the README's own (default) architecture and settings
            _log("secondary: README default architecture")
            result["readme_default_arch"] = G2C.train_cfg3(dev, 0.1, arch="mlp", H=64, forward_too=True)
            torch.cuda.empty_cache()
        if sharded_leg and args.workload == "cfg3":
            # N = 1: the cfg5 shard through the dst-range code path (world-1 process group over RCCL, nothing cut), after
            # every launch-bound measurement of the run
            sharded_variants()
        if args.full and not args.no_cpu_baseline:
            _log("cpu baseline (thread sweep) + full-size parity")
            first = (lambda: G2C.step_cfg3(st)) if rotation is not None else step     # parity: the FIRST minibatch of the rotation
            with torch.no_grad():
                gpu_out = first()
            gpu_out = gpu_out.output_node_representations if args.workload == "cfg3" else gpu_out
            base, parity = (CPU.cpu_baseline_cfg2 if args.workload == "cfg2" else CPU.cpu_baseline_cfg3)(st, gpu_out)
            parity["strict_1e-5"] = bool(parity["max_abs"] <= C.PARITY_TOL)
            result["cpu_baseline"] = base
            # every config the run checked, rolled up: `strict_1e-5` (AND) and who passes on the float64-attributed bar only
            result["parity"] = C.parity_rollup(parity, parities)
            if not parity["max_abs"] <= C.PARITY_TOL:
                exit_code = 3
    if C.have_group():
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    _log("done")
    if rank == 0:      # the one line of stdout (C.hold_stdout parked everything else, RCCL's banner included, on stderr)
        C.emit_line(json.dumps(result))
    if exit_code:
        sys.stderr.write("bench.py: GPU output is outside the parity tolerance of the CPU oracle (see \"parity\")\n")
        sys.exit(exit_code)


if __name__ == "__main__":
    main()
