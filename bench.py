#!/usr/bin/env python3
"""bench.py -- unlabelled-pool images/sec scored (ENet, 1024x2048) on N MI355X GPUs.

Headline workload (BASELINE.json configs[1] / [2]): a pool of 2975 synthetic Cityscapes-shaped frames
(1024x2048x3 fp32 NHWC, device-resident before the timed region), ENet(19 classes) with seeded
synthetic weights, entropy acquisition, batches of 8 (reference conf/*.json:2).  One "step" = one
batch of 8 frames through the fused path: ENet forward + per-pixel softmax-entropy + float64
per-image mean.  With N > 1 the pool is sharded over the ranks (one process per GPU) and the per-image
(index, score) pairs are merged by ONE RCCL all-gather followed by the float32 scatter + top-128
argpartition on every rank; that merge is inside the timed region.

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Scaling mode: N = 1 times exactly K steps.  N > 1 defaults to STRONG scaling, the statement north_star / SURVEY 8(d)
make ("images/s = 2975 / t", ">= 6x at 8 GPUs"): the fixed 2975-frame pool is split over the ranks, `value` = 2975 /
max-over-ranks time, `steps` = the batches each rank ran (`requested_steps` keeps K); with `--full` the weak figure
(every rank scores exactly K batches of its shard) is timed right after and reported beside it as `weak`.
`--scaling weak` makes the weak figure the headline instead.

A plain run sets up, warms up, times the K steps, writes the outputs of the timed path when `--dump-outputs DIR` is
given, and prints ONE JSON line with the headline (`metric`, `value`, `unit`, `higher_is_better`, `dtype`,
`ms_per_step`, ...).  Everything else is measured or checked only with `--full`:

    python bench.py --full [--no-roofline] [--no-secondary] [--no-cpu-baseline]

`--dump-outputs DIR` (after the timed steps, rank 0): what the timed path returned, as float64 .npy files --
`scores.npy` / `frame_ids.npy` (the per-image scores of the last timed step and the frames they belong to),
`top_k.npy` (the sorted top-128 selection made by the merge that closes the timed region) and `pool_frame_ids.npy` /
`pool_scores.npy` (every frame the timed region scored, once, in frame-id order; at most the 2975 pool frames).
The inputs are seeded synthetic frames and weights, so the same arguments give the same inputs on every run.

With `--full`, rank 0's line also carries
  `weak`            (N > 1, strong scaling) the weak figure, timed right after the strong one,
  `roofline`        dominant kernel, HIP-event timed live on the launch stream in a separate profiling pass,
  `roofline_all`    the same figures for EVERY kernel symbol of the pass (avg us, algorithmic flops / bytes per launch,
                    bound, frac, PMC traffic per launch from the committed profiles/<round>_pmc passes),
  `score_digest`    SHA-256 of the float64 scores of the frames scored in the timed region, compared with the digest of
                    the same frames in the committed table tests/golden/pool_scores.npz; a mismatch makes the bench exit
                    non-zero.  The table is a REGRESSION PIN produced by the HIP path itself (tools/make_pool_scores.py),
                    not oracle parity: what ties it to the C oracle is one frame per table (index 100) that the parity
                    tests check against the oracle AND against the table entry, bit for bit,
  `secondary`       (N = 1) short legs of the other single-GPU BASELINE configs: c4 = configs[3] ICNet / margin,
                    c5 = configs[4] ENet RGB+NIR, 6 classes / entropy -- each with value, ms_per_step, roofline, digest,
  `cpu_baseline`    the torch-CPU restatement of the reference path, timed on this box's host cores (N = 1 only),
and writes the full result to the detail file it names (a plain run writes one only when `--detail-file` is given).
"""
import argparse
import datetime
import hashlib
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
# the host driver of the GPU pool only supports dmabuf IPC: RCCL / device-tensor sharing across the ranks of one node
# needs this before the HIP runtime comes up (it is exported on the pool already; kept here for any other launcher)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
# streams -> hardware queues: the HIP runtime's default cap is 4 per process; the image-group schedule uses the caller's
# stream + 2 side streams, an N > 1 rank adds RCCL's stream (and a prefetch stream in the real ranking loop).  Measured on
# one GPU (profiles/r04_ab_hw_queues.txt): 4, 8 and 16 queues score the same, 2 (or an empty value) lose 11 %.
# The PACKAGE defaults both variables at import (semanticsegmentationactivelearning_amd/_lib.py) -- a ranking job that
# imports it gets what this bench measures; the line's knobs.env names the values and which of them were injected.
if not os.environ.get("GPU_MAX_HW_QUEUES"):
    os.environ["GPU_MAX_HW_QUEUES"] = "8"
    os.environ["SSAL_BENCH_INJECTED_HWQ"] = "1"

POOL = 2975          # Cityscapes train split size (BASELINE.json configs[1])
TOP_K = 128          # BASELINE.json configs[2]
HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec)
FP32_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: fp32 vector == fp32-input MFMA peak
BF16_PEAK_TFLOPS = 2516.8  # MI355X_MICROARCH.md: dense bf16 MFMA peak (v_mfma_f32_32x32x16_bf16: 16384 MACs in 8 passes)
BF16X3_PRODUCTS = 6        # the opt-in mode executes six bf16 MFMAs per fp32-equivalent K step (csrc/ssal_bottleneck_bf16x3.hip)
MEASURED_FP32_TFLOPS = 155.0  # bare v_mfma_f32_32x32x2 chains on this part (profiles/r04_probe_mfma_peak_and_bf16x3_split.txt)
MEASURED_HBM_GBS = 6300.0     # best tile-organised copy on this part (tools/hbm_bw.py, profiles/r02_probes.txt)
SCORE_TABLE = os.path.join(ROOT, "tests", "golden", "pool_scores.npz")
PMC_ROUNDS = ("r05", "r04", "r03", "r02")  # newest committed PMC pass first
DETAIL_FILE = os.path.join(ROOT, "gpurun_out", "bench_detail.json")
ICNET_NOTE = ("ICNet as pinned by ICNET_SPEC.md -- the reference's models/icnet/icnet.py is an empty class: parity "
              "unpinned AND undefined")


def log(msg):
    """progress on stderr (stdout carries exactly one JSON line)"""
    if os.environ.get("RANK", "0") == "0":
        print("[bench %7.1fs] %s" % (time.perf_counter() - _T0, msg), file=sys.stderr, flush=True)


_T0 = time.perf_counter()


class Watchdog:
    """`with Watchdog(seconds, what):` -- if the block has not finished after `seconds`, say so on stderr and leave the
    process with exit code 3 (a rank that never arrives must not hang the job: collectives block inside C code, so
    an exception cannot be raised into them; os._exit is the only way out)."""

    def __init__(self, seconds, what):
        self.seconds, self.what, self._done = float(seconds), what, threading.Event()

    def _run(self):
        if not self._done.wait(self.seconds):
            print("[bench] TIMEOUT after %.0f s in: %s (rank %s of %s) -- a rank is missing or hung; exiting 3"
                  % (self.seconds, self.what, os.environ.get("RANK", "0"), os.environ.get("WORLD_SIZE", "1")),
                  file=sys.stderr, flush=True)
            os._exit(3)

    def __enter__(self):
        if self.seconds > 0:
            threading.Thread(target=self._run, daemon=True).start()
        return self

    def __exit__(self, *exc):
        self._done.set()
        return False


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=372)   # 372 batches of 8 = the whole 2975-frame pool
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--classes", type=int, default=19)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--model", choices=["enet", "icnet"], default="enet",
                    help="enet: BASELINE configs[1] (the metric's workload); icnet: configs[3] (ICNet multi-scale, "
                         "margin), architecture pinned in ICNET_SPEC.md")
    ap.add_argument("--measure", default=None, help="entropy | margin | confidence (default: entropy, margin for icnet)")
    ap.add_argument("--arithmetic", choices=["f32", "bf16x3"], default="f32",
                    help="MEASUREMENT runs of the opt-in mode only (profiles of its kernels): the main leg scores with "
                         "ENet.score(arithmetic=...).  The default f32 is the reference's arithmetic and the only headline; a "
                         "bf16x3 line says so in metric / dtype / config and checks its scores against the exact table within 1e-6")
    ap.add_argument("--weights-seed", type=int, default=0)
    ap.add_argument("--input-dtype", choices=["f32", "u8"], default="f32",
                    help="resident frames: float32 in [0,1] (the reference's model input) or the decoded uint8 "
                         "frames, converted inside the Initial kernel (same bits out)")
    ap.add_argument("--resident-gib", type=float, default=96.0,
                    help="cap on device memory used for resident input frames (wraps beyond it)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the weak figure beside a strong one, the roofline leg, the secondary legs, "
                         "the CPU baseline, the score digest against the committed table and the detail file (the --no-* "
                         "options below switch single parts off)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the timed path returned as DIR/<name>.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the C4 / C5 legs (profiling runs)")
    ap.add_argument("--secondary-steps", type=int, default=24)
    ap.add_argument("--scaling", choices=["weak", "strong"], default=None,
                    help="default: strong when WORLD_SIZE > 1 (the fixed 2975-frame pool split over the ranks, value = "
                         "2975 / t; the weak figure is reported beside it), weak at N = 1 (exactly --steps steps)")
    ap.add_argument("--dist-timeout", type=float, default=180.0,
                    help="seconds a rendezvous / barrier / collective may take before the process exits non-zero")
    ap.add_argument("--allow-nondefault-knobs", action="store_true",
                    help="measurement runs only (tools/*.sh with a -DSSAL_MEASURE library): time the library although "
                         "ssal_debug_get_knobs() says a switch is off its default; the JSON line still reports them")
    ap.add_argument("--knob", action="append", default=[], metavar="NAME=VALUE",
                    help="measurement runs only: ssal_debug_set_knob(NAME, VALUE) before anything is timed (needs "
                         "--allow-nondefault-knobs; the JSON line reports the knobs)")
    ap.add_argument("--detail-file", default=None,
                    help="full result (per-kernel flops / bytes / traffic, whole secondary legs); the stdout line carries "
                         "the compact form and names this file (default with --full: DETAIL_FILE)")
    ap.add_argument("--full-line", action="store_true",
                    help="tools/*.sh: print the full result object on stdout instead of the compact line")
    ap.add_argument("--allow-digest-mismatch", action="store_true",
                    help="measurement builds whose results are invalid by construction (ablation): report, do not fail")
    return ap.parse_args(argv)


# ---- score table / digest ---------------------------------------------------------------------------------
def table_key(model, c, classes, h, w, measure, seed):
    return "%s_c%dk%d_%dx%d_%s_seed%d" % (model, c, classes, h, w, measure, seed)


def load_score_table(key):
    try:
        with np.load(SCORE_TABLE) as z:
            return np.array(z[key], dtype=np.float64) if key in z.files else None
    except Exception:
        return None


def unique_frames(index, score):
    """(frame ids, scores) of the frames scored, once each, in frame-id order (a wrapped batch list may score a frame
    twice: same bits, keep one; padding entries of a short shard have index -1)"""
    index = np.asarray(index, dtype=np.int64)
    score = np.asarray(score, dtype=np.float64)
    keep = index >= 0
    index, score = index[keep], score[keep]
    first = np.unique(index, return_index=True)[1]
    return index[first], score[first]


def score_digest(index, score, key):
    """SHA-256 of the float64 scores (frame-id order) of the frames actually scored, vs the committed table"""
    index, score = unique_frames(index, score)
    out = {"frames": int(len(index)), "sha256": hashlib.sha256(np.ascontiguousarray(score).tobytes()).hexdigest(),
           "table": "tests/golden/pool_scores.npz[%s]" % key, "expected_sha256": None, "match": None}
    table = load_score_table(key)
    if table is not None and len(index) and index.max() < len(table):
        want = table[index]
        out["expected_sha256"] = hashlib.sha256(np.ascontiguousarray(want).tobytes()).hexdigest()
        out["match"] = bool(out["sha256"] == out["expected_sha256"])
        out["max_abs_diff"] = float(np.max(np.abs(score - want)))
    return out


def dump_outputs(head, out_dir):
    """--dump-outputs: what the timed path returned, as float64 arrays (at most a few POOL-sized vectors, ~100 KB)"""
    ids, scores = head["last_step"]
    pool_ids, pool_scores = unique_frames(head["index"], head["score"])
    arrays = {"scores": scores.cpu().numpy(), "frame_ids": ids.cpu().numpy(), "top_k": np.sort(head["low"]),
              "pool_frame_ids": pool_ids, "pool_scores": pool_scores}
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))
    log("outputs of the timed path written to %s (%s)" % (out_dir, ", ".join(sorted(arrays))))


# ---- CPU baseline -----------------------------------------------------------------------------------------
CPU_REPEATS = 12  # fixed sample: 1 warm-up + 12 single-frame passes (~0.9 s each on a 16-thread share: 10-15 s)


def cpu_baseline(P, h, w, c, measure, budget_s, c1=None, model="enet"):
    """torch-CPU restatement of the reference path (oracle/torch_restatement.py) on a bounded, FIXED sample: single
    1024x2048 frames, 1 warm-up + CPU_REPEATS passes (cut short only if one pass takes so long that the sample would
    exceed 4x the budget); `value` is the MEDIAN pass, min / max are reported beside it -- the GPU box's host cores are
    shared, and two runs of one build have differed 1.7x when the sample size followed the clock."""
    import torch
    from oracle import torch_restatement as tr
    from oracle.enet_oracle import usable_cores
    from semanticsegmentationactivelearning_amd import synthetic as syn
    cores = usable_cores()
    torch.set_num_threads(cores)
    log("cpu baseline: %d threads (affinity %d, cpu_count %s)" % (cores, len(os.sched_getaffinity(0)), os.cpu_count()))
    x = syn.synth_frames_f32([0], h, w, c)
    score_images = tr.icnet_score_images if model == "icnet" else tr.score_images
    t0 = time.perf_counter()
    score_images(P, x, measure)  # warm-up
    log("cpu baseline warm-up %.2f s" % (time.perf_counter() - t0))
    times = []
    t_all = time.perf_counter()
    while len(times) < CPU_REPEATS:
        t0 = time.perf_counter()
        score_images(P, x, measure)
        times.append(time.perf_counter() - t0)
        log("cpu baseline run %d: %.2f s" % (len(times), times[-1]))
        if len(times) >= 2 and (time.perf_counter() - t_all) > 4.0 * budget_s:
            break
    med = float(np.median(times))
    out = {"value": 1.0 / med, "unit": "images/s", "cores": int(torch.get_num_threads()), "kind": "port",
           "min": 1.0 / max(times), "median": 1.0 / med, "max": 1.0 / min(times), "repeats": len(times),
           "sample": "%d x 1 frame %dx%dx%d forward+%s score, torch-CPU fp32 restatement of the reference "
                     "TF path (TensorFlow itself is not installable here), median of %d runs after 1 warm-up"
                     % (len(times), h, w, c, measure, len(times))}
    if c1 is not None:
        # BASELINE.json configs[0] / SURVEY 8(d): the reference's own CPU-runnable case, timed exactly:
        # 4 x 256x512x3 frames -> forward + entropy score + top-1 select
        P1, k1 = c1
        x1 = syn.synth_frames_f32([0, 1, 2, 3], 256, 512, 3)
        tr.score_images(P1, x1, "entropy")
        t1 = []
        while len(t1) < 3 or sum(t1) < 3.0:
            t0 = time.perf_counter()
            mean = tr.score_images(P1, x1, "entropy")[0]
            np.argpartition(np.asarray(mean, dtype=np.float32), 1)[:1]
            t1.append(time.perf_counter() - t0)
            if len(t1) >= 30:
                break
        m1 = float(np.median(t1))
        log("cpu baseline C1 (4 x 256x512): %.3f s" % m1)
        out["c1"] = {"value": 4.0 / m1, "unit": "images/s", "cores": int(torch.get_num_threads()), "kind": "port",
                     "sample": "configs[0]: %d x (4 frames 256x512x3, K=%d: forward + entropy + top-1), median"
                               % (len(t1), k1)}
    return out


# ---- roofline ---------------------------------------------------------------------------------------------
def load_pmc(model):
    for rnd in PMC_ROUNDS:
        try:
            pmc = json.load(open(os.path.join(ROOT, "profiles", "%s_pmc" % rnd, "traffic_%s.json" % model)))
        except Exception:
            continue
        try:  # the opt-in bf16x3 kernels have their own PMC pass (tools/refresh_profiles.sh)
            extra = json.load(open(os.path.join(ROOT, "profiles", "%s_pmc" % rnd, "traffic_%s_bf16x3.json" % model)))
            pmc.update({k: v for k, v in extra.items() if "bf16x3" in k})
        except Exception:
            pass
        return rnd, pmc
    return None, {}


def kernel_roofline(name, d, reps, pmc):
    """one profile row -> roofline figures; d = {"launches", "ms", "flops", "bytes"} summed over `reps` batches"""
    sec = d["ms"] * 1e-3
    n = max(d["launches"], 1)
    # rows of the opt-in bf16x3 kernels: the launcher reports fp32-EQUIVALENT flops; what the matrix pipe executes is six
    # bf16 products per fp32 product, priced against the dense bf16 peak
    split = "bf16x3" in name
    flop_peak = BF16_PEAK_TFLOPS if split else FP32_PEAK_TFLOPS
    if split:
        d = dict(d, flops=d["flops"] * BF16X3_PRODUCTS)
    ridge = flop_peak * 1e12 / (HBM_PEAK_GBS * 1e9)
    ai = d["flops"] / d["bytes"] if d["bytes"] > 0 else float("inf")
    if d["bytes"] <= 0 and d["flops"] <= 0:
        bound, achieved, peak, unit = "latency", None, None, None
    elif ai >= ridge:
        bound, achieved, peak, unit = "mfma", d["flops"] / sec / 1e12, flop_peak, "TFLOP/s"
    else:
        bound, achieved, peak, unit = "hbm", d["bytes"] / sec / 1e9, HBM_PEAK_GBS, "GB/s"
    traffic = pmc.get("hbm_bytes_per_launch") if pmc else None
    # "mfma" is the schema's name for the compute roof; the fp32 VECTOR peak equals the fp32 MFMA peak on this part
    # (157.3 TFLOP/s), and these two kernels run their FLOPs on packed VALU FMAs, not on the matrix cores
    pipe = "mfma bf16 (6 products per fp32 product)" if split else None if bound != "mfma" else ("valu (v_pk_fma_f32)" if name.startswith(("k_final_score", "k_upscore", "k_conv_first"))
                                         else "valu (v_pk_fma_f32) conv 1 + mfma conv 2" if name.startswith("k_front2") else "mfma")
    return {"bound": bound, "pipe": pipe, "achieved": achieved, "peak": peak, "unit": unit,
            "frac": (achieved / peak) if achieved is not None else None, "traffic": traffic,
            "traffic_over_algorithmic": (traffic / (d["bytes"] / n)) if (traffic and d["bytes"] > 0) else None,
            "avg_us": 1e3 * d["ms"] / n, "launches_per_batch": d["launches"] // reps,
            "flops": d["flops"] / n, "bytes": d["bytes"] / n, "ms_per_batch": d["ms"] / reps}


def roofline_leg(net, batch, measure, model, reps=3, arithmetic="f32"):
    """separate pass, outside every timed region: ssal_profile_enable(1) brackets each launch with HIP events on the
    launch stream.  -> (roofline of the dominant kernel, roofline_all)"""
    import torch
    from semanticsegmentationactivelearning_amd import _lib
    _lib.profile_enable(True)
    try:
        kw = {} if arithmetic == "f32" else {"arithmetic": arithmetic}
        for _ in range(reps):
            net.score(batch, measure=measure, **kw)
        torch.cuda.synchronize()
        prof = _lib.profile_collect()
    finally:
        _lib.profile_enable(False)
    rnd, pmc = load_pmc(model)
    rows = {k: kernel_roofline(k, v, reps, pmc.get(k)) for k, v in sorted(prof.items())}
    dom = max(prof, key=lambda k: prof[k]["ms"])
    d, r = prof[dom], rows[dom]
    total_ms = sum(v["ms"] for v in prof.values())
    sec = d["ms"] * 1e-3
    roof = {"kernel": dom, "bound": r["bound"], "achieved": r["achieved"], "peak": r["peak"], "unit": r["unit"],
            "frac": r["frac"], "traffic": r["traffic"], "traffic_source": ("profiles/%s_pmc" % rnd) if rnd else None,
            "algorithmic_bytes_per_launch": r["bytes"], "algorithmic_flops_per_launch": r["flops"],
            "avg_launch_us": r["avg_us"], "launches_per_batch": r["launches_per_batch"],
            "share_of_gpu_time": d["ms"] / total_ms,
            "arithmetic_intensity_flop_per_byte": d["flops"] / d["bytes"] if d["bytes"] > 0 else None,
            "achieved_tflops": d["flops"] / sec / 1e12, "achieved_gbs": d["bytes"] / sec / 1e9,
            "per_kernel_ms_per_batch": {k: v["ms"] / reps for k, v in sorted(prof.items())}}
    # whole pass against the sum of its kernels' binding floors
    floor_ms = 0.0
    for k, v in prof.items():
        fsec = v["flops"] * BF16X3_PRODUCTS / (BF16_PEAK_TFLOPS * 1e12) if "bf16x3" in k else v["flops"] / (FP32_PEAK_TFLOPS * 1e12)
        floor_ms += max(fsec, v["bytes"] / (HBM_PEAK_GBS * 1e9)) * 1e3 / reps
    roof["schedule"] = ("whole-batch launches on one stream (ssal_profile_enable serialises the image-group chains the "
                        "timed region overlaps): each kernel is timed alone on the chip")
    roof["pass_ms_per_batch"] = total_ms / reps
    roof["pass_floor_ms_per_batch"] = floor_ms
    roof["pass_frac_of_kernel_floors"] = floor_ms / (total_ms / reps) if total_ms > 0 else None
    # the whole pass against the two roofs at their MEASURED peaks: if arithmetic and traffic did not overlap at all the
    # batch would take flops_ms + bytes_ms (no-overlap bound), with perfect overlap max(flops_ms, bytes_ms)
    fl_ms = sum(v["flops"] for v in prof.values()) / reps / (MEASURED_FP32_TFLOPS * 1e12) * 1e3
    by_ms = sum(v["bytes"] for v in prof.values()) / reps / (MEASURED_HBM_GBS * 1e9) * 1e3
    nimg = int(batch.shape[0])
    roof["pass_flops_ms"], roof["pass_bytes_ms"] = fl_ms, by_ms
    roof["pass_no_overlap_bound"] = {"ms_per_batch": fl_ms + by_ms, "images_per_s": 1e3 * nimg / (fl_ms + by_ms)}
    roof["pass_overlap_bound"] = {"ms_per_batch": max(fl_ms, by_ms), "images_per_s": 1e3 * nimg / max(fl_ms, by_ms)}
    roof["pass_bounds_peaks"] = "measured: %.0f TFLOP/s fp32 MFMA, %.1f TB/s HBM" % (MEASURED_FP32_TFLOPS, MEASURED_HBM_GBS / 1e3)
    return roof, rows


# ---- the printed line ---------------------------------------------------------------------------------------
LINE_LIMIT = 6000  # bytes: the driver keeps a bounded tail of stdout; round 3's 16 KB line lost secondary.c4 there


def _r(v, nd=4):
    return round(v, nd) if isinstance(v, float) else v


def compact_rows(rows):
    """roofline_all of the printed line: {kernel: {n = launches per batch, avg_us, frac, bound, traffic_over_algorithmic}}"""
    return {k: {"n": v["launches_per_batch"], "avg_us": _r(v["avg_us"], 1), "frac": _r(v["frac"], 3), "bound": v["bound"],
                "traffic_over_algorithmic": _r(v["traffic_over_algorithmic"], 2)} for k, v in rows.items()}


def compact_roofline(roof):
    """the contract's roofline object + what locates it (kernel, launch time, share); the rest lives in the detail file"""
    keep = ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "avg_launch_us",
            "launches_per_batch", "share_of_gpu_time", "algorithmic_bytes_per_launch", "algorithmic_flops_per_launch",
            "pass_ms_per_batch", "pass_frac_of_kernel_floors", "pass_no_overlap_bound", "pass_overlap_bound")
    out = {k: _r(roof[k], 4) for k in keep if k in roof}
    for k in ("pass_no_overlap_bound", "pass_overlap_bound"):
        if k in out:
            out[k] = {kk: _r(vv, 3) for kk, vv in out[k].items()}
    return out


def compact_line(full, detail_path):
    """the ONE stdout line (<= LINE_LIMIT bytes): contract fields, compact roofline rows, short secondary legs; everything
    else is in `detail_path` (full per-kernel figures, full secondary legs, per-kernel ms per batch)"""
    line = {k: v for k, v in full.items() if k not in ("roofline", "roofline_all", "secondary", "cpu_baseline")}
    if "roofline" in full:
        line["roofline"] = compact_roofline(full["roofline"])
    if "roofline_all" in full:
        line["roofline_all"] = compact_rows(full["roofline_all"])
    if "secondary" in full:
        line["secondary"] = {}
        for nm, sec in full["secondary"].items():
            d = {"value": _r(sec["value"], 1), "unit": sec["unit"], "ms_per_step": _r(sec["ms_per_step"], 4),
                 "steps": sec["steps"], "digest_match": sec["score_digest"]["match"], "config": sec["config"].split(";")[0][:80],
                 "parity": "unpinned AND undefined (no reference ICNet exists: ICNET_SPEC.md)" if "undefined" in sec["config"]
                           else "unpinned (no TensorFlow, no reference fixtures)"}
            if sec.get("arithmetic"):
                d["dtype"] = sec["dtype"]
                d["max_abs_score_diff_vs_exact"] = _r(sec["score_digest"].get("max_abs_diff"), 10)
                d["parity"] = "opt-in mode, not the reference's arithmetic: scores within 1e-6 of the exact path; " + d["parity"]
                if "roofline_bf16x3" in sec:
                    rb = sec["roofline_bf16x3"]
                    d["roofline_bf16x3"] = {"kernel": rb["kernel"], "bound": rb["bound"], "achieved": _r(rb["achieved"], 1),
                                            "peak": rb["peak"], "unit": rb["unit"], "frac": _r(rb["frac"], 3),
                                            "avg_us": _r(rb["avg_us"], 1), "n": rb["launches_per_batch"]}
            if "roofline" in sec:
                d["dominant_kernel"] = sec["roofline"]["kernel"]
                d["dominant_frac"] = _r(sec["roofline"]["frac"], 3)
                d["dominant_avg_us"] = _r(sec["roofline"]["avg_launch_us"], 1)
                d["pass_frac_of_kernel_floors"] = _r(sec["roofline"]["pass_frac_of_kernel_floors"], 3)
            line["secondary"][nm] = d
    if "cpu_baseline" in full:
        line["cpu_baseline"] = full["cpu_baseline"]
    line["detail_file"] = os.path.relpath(detail_path, ROOT) if detail_path else None
    text = json.dumps(line)
    if len(text) > LINE_LIMIT:  # never print a line the driver would cut: drop the widest optional parts first
        for victim in ("roofline_all", "knobs"):
            line.pop(victim, None)
            text = json.dumps(line)
            if len(text) <= LINE_LIMIT:
                break
    return text


def write_detail(full, path):
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(full, f, indent=1, sort_keys=True)
        return path
    except OSError as e:  # a read-only checkout must not cost the bench line
        log("detail file not written (%s)" % e)
        return None


# ---- one scoring leg ----------------------------------------------------------------------------------------
class Leg:
    """model + resident shard batches + the timed ranking pass over them"""

    def __init__(self, args, ctx, model, classes, c, measure, seed, input_dtype="f32", arithmetic="f32"):
        import torch
        import semanticsegmentationactivelearning_amd as ssal
        from semanticsegmentationactivelearning_amd import synthetic as syn
        self.args, self.ctx, self.model, self.classes, self.c, self.measure, self.seed = args, ctx, model, classes, c, measure, seed
        self.h, self.w, self.bs = args.height, args.width, args.batch
        if model == "icnet":
            self.net = ssal.ICNet(classes)
            self.net.build((None, None, None, c))
            syn.randomize_icnet(self.net, seed=seed)
        else:
            self.net = ssal.ENet(classes)
            self.net.build((None, None, None, c))
            syn.randomize_enet(self.net, seed=seed)
        self.torch, self.syn = torch, syn
        self.input_dtype = input_dtype
        self.arithmetic = arithmetic  # "f32" (headline, every default leg) or ENet's opt-in "bf16x3" (secondary.c2_bf16x3 only)
        self.batches = []

    def make_resident(self, n_batches):
        """this rank's strided shard of the pool, device-resident before any clock starts"""
        from semanticsegmentationactivelearning_amd import active_learning as al
        torch, syn, ctx = self.torch, self.syn, self.ctx
        positions = al.shard_positions(POOL, ctx["rank"], ctx["world"])
        self.positions = positions[positions >= 0]
        self.n_batches_shard = (len(self.positions) + self.bs - 1) // self.bs
        in_dtype = torch.uint8 if self.input_dtype == "u8" else torch.float32
        bytes_per_batch = self.bs * self.h * self.w * self.c * (1 if self.input_dtype == "u8" else 4)
        max_resident = max(1, int(self.args.resident_gib * 2 ** 30 // bytes_per_batch))
        n_resident = min(n_batches, self.n_batches_shard, max_resident)
        for b in range(len(self.batches), n_resident):
            ids = self.positions[b * self.bs:(b + 1) * self.bs]
            buf = torch.empty((len(ids), self.h, self.w, self.c), dtype=in_dtype, device=ctx["dev"])
            # strided shard: frame ids are not consecutive when world > 1 -> one generator call per frame
            if ctx["world"] == 1:
                syn.synth_frames_device(int(ids[0]), len(ids), self.h, self.w, self.c, out=buf)
            else:
                for j, f in enumerate(ids):
                    syn.synth_frames_device(int(f), 1, self.h, self.w, self.c, out=buf[j:j + 1])
            self.batches.append((buf, torch.as_tensor(ids, device=ctx["dev"])))
        torch.cuda.synchronize()
        self.bytes_per_batch = bytes_per_batch
        return len(self.batches)

    def run_steps(self, k, first):
        torch = self.torch
        idx_chunks, score_chunks, frames = [], [], 0
        for s in range(k):
            xb, ib = self.batches[(first + s) % len(self.batches)]
            if self.arithmetic == "f32":
                score_chunks.append(self.net.score(xb, measure=self.measure))
            else:
                score_chunks.append(self.net.score(xb, measure=self.measure, arithmetic=self.arithmetic))
            idx_chunks.append(ib)
            frames += xb.shape[0]
        self.last_step = (idx_chunks[-1], score_chunks[-1]) if k else None  # what the last step returned (--dump-outputs)
        return torch.cat(idx_chunks), torch.cat(score_chunks), frames

    def merge_and_select(self, index, score, pad_steps):
        """ONE collective: every rank pads its (index, score) shard locally to pad_steps * batch entries (the same number on
        every rank; a shard's last batch may be short) and all-gathers it; then the float32 scatter + top-k on the host"""
        from semanticsegmentationactivelearning_amd import active_learning as al
        if self.ctx["use_dist"]:
            index, score = al.pad_to_length(index, score, pad_steps * self.bs)
        all_index, all_score = al.all_gather_scores(index, score)
        all_index, all_score = all_index.cpu().numpy(), all_score.cpu().numpy()
        low, _ = al.finish_ranking(all_index, all_score, POOL, np.arange(POOL), TOP_K)
        return low, all_index, all_score

    def timed(self, steps, first, what):
        """barrier + synchronize | exactly `steps` steps + the merge | synchronize + barrier; max over ranks"""
        import torch.distributed as dist
        torch, ctx = self.torch, self.ctx
        with Watchdog(self.args.dist_timeout + 60.0 + 0.1 * steps, "timed region (%s)" % what):
            if ctx["use_dist"]:
                dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            index, score, frames = self.run_steps(steps, first)
            low, all_index, all_score = self.merge_and_select(index, score, steps)
            torch.cuda.synchronize()
            if ctx["use_dist"]:
                dist.barrier()
            elapsed = time.perf_counter() - t0
            t = torch.tensor([elapsed, float(frames)], dtype=torch.float64,
                             device="cpu" if ctx["backend"] == "gloo" else ctx["dev"])
            if ctx["use_dist"]:
                tmax = t.clone()
                dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
                dist.all_reduce(t, op=dist.ReduceOp.SUM)
                elapsed, total_frames = float(tmax[0]), float(t[1])
            else:
                total_frames = float(frames)
        log("%s: %d steps, %.0f frames over all ranks in %.3f s (max over ranks)" % (what, steps, total_frames, elapsed))
        return {"elapsed": elapsed, "frames": total_frames, "steps": steps, "low": low,
                "index": all_index, "score": all_score, "last_step": self.last_step}

    def key(self):
        return table_key(self.model, self.c, self.classes, self.h, self.w, self.measure, self.seed)


def init_distributed(args):
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if args.gpus > 1 and world == 1:
        raise SystemExit("launch with torch.distributed.run for --gpus > 1")
    assert torch.cuda.is_available(), "bench.py needs MI355X GPUs (no CPU fallback)"
    # SSAL_DIST_BACKEND=gloo: rehearsal of the multi-rank path on a box with fewer GPUs than ranks (ranks share
    # the cards round-robin, collectives run on CPU tensors); the real run is one rank per GPU over RCCL
    backend = os.environ.get("SSAL_DIST_BACKEND", "nccl")
    dev_index = local_rank % torch.cuda.device_count() if backend == "gloo" else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    # launched through torch.distributed.run: initialise the process group even for ONE rank, so that the single-GPU
    # rehearsal of the launcher command exercises the RCCL branch (init with device_id, barriers, reductions)
    use_dist = world > 1 or os.environ.get("TORCHELASTIC_RUN_ID") is not None
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # RCCL prints its banner (host name, library path) on the C-level stdout when the communicator comes up:
        # stdout carries exactly ONE JSON line, so fd 1 points at stderr until the first collective has run
        sys.stdout.flush()
        saved_fd = os.dup(1)
        os.dup2(2, 1)
        try:
            # a rank that never shows up: the rendezvous raises after --dist-timeout (-> non-zero exit); a rank that
            # hangs later is caught by the Watchdog around every barrier / timed region
            tmo = datetime.timedelta(seconds=args.dist_timeout)
            with Watchdog(args.dist_timeout + 30.0, "init_process_group + first barrier"):
                if backend == "gloo":
                    dist.init_process_group("gloo", timeout=tmo)
                else:
                    dist.init_process_group("nccl", device_id=dev, timeout=tmo)  # nccl == RCCL on ROCm
                dist.barrier()
                torch.cuda.synchronize()
        finally:
            sys.stdout.flush()
            os.dup2(saved_fd, 1)
            os.close(saved_fd)
    return {"world": world, "rank": rank, "dev": dev, "backend": backend, "use_dist": use_dist}


def secondary_leg(args, ctx, name, model, classes, c, measure, seed, note, arithmetic="f32"):
    """a short N = 1 leg of another BASELINE config: value, ms_per_step, roofline, roofline_all, digest"""
    import torch
    steps, warm = max(1, args.secondary_steps), 2
    leg = Leg(args, ctx, model, classes, c, measure, seed, arithmetic=arithmetic)
    leg.make_resident(steps + warm)
    i0, s0, _ = leg.run_steps(warm, 0)
    leg.merge_and_select(i0, s0, warm)
    torch.cuda.synchronize()
    r = leg.timed(steps, warm, "secondary %s" % name)
    out = {"config": note, "value": r["frames"] / r["elapsed"], "unit": "images/s", "steps": steps, "warmup": warm,
           "ms_per_step": 1e3 * r["elapsed"] / steps, "dtype": "f32", "data": "synthetic",
           "score_digest": score_digest(r["index"], r["score"], leg.key())}
    if arithmetic != "f32":
        # NOT the reference's arithmetic: its scores are not the committed table's bits; the check is the mode's own gate
        # (tests/test_gpu_bf16x3.py): every per-image score within 1e-6 of the exact path's table entry
        dg = out["score_digest"]
        out["dtype"] = "f32 via bf16x3 (6 products, fp32 accumulate)"
        out["arithmetic"] = arithmetic
        dg["tolerance"] = 1e-6
        dg["within_tolerance"] = bool(dg.get("max_abs_diff") is not None and dg["max_abs_diff"] <= 1e-6)
        dg["match"] = dg["within_tolerance"]  # the verdict of THIS leg: within its stated tolerance of the exact table
        dg["bit_identical_to_table"] = bool(dg["sha256"] == dg["expected_sha256"])
    if not args.no_roofline:
        out["roofline"], out["roofline_all"] = roofline_leg(leg.net, leg.batches[0][0], measure, model, arithmetic=arithmetic)
        if arithmetic != "f32":  # this leg's own row: the dominant kernel OF THE MODE
            split = {k: v for k, v in out["roofline_all"].items() if "bf16x3" in k}
            if split:
                kname = max(split, key=lambda k: split[k]["ms_per_batch"])
                out["roofline_bf16x3"] = dict(split[kname], kernel=kname)
    del leg
    torch.cuda.empty_cache()
    return out


def main(argv=None):
    args = parse(argv)
    import torch
    import torch.distributed as dist

    import semanticsegmentationactivelearning_amd as ssal
    from semanticsegmentationactivelearning_amd import _lib, synthetic as syn

    ctx = init_distributed(args)
    world, rank, use_dist = ctx["world"], ctx["rank"], ctx["use_dist"]
    scaling = args.scaling or ("strong" if world > 1 else "weak")

    for kv in args.knob:
        name, value = kv.split("=", 1)
        _lib.set_knob(name, int(value))
    knobs = _lib.get_knobs()
    if not knobs["defaults"] and not args.allow_nondefault_knobs:
        raise SystemExit("refusing to time a library whose switches are not at their shipping values: %s" % knobs)

    h, w, c, bs = args.height, args.width, args.channels, args.batch
    if args.measure is None:
        args.measure = "margin" if args.model == "icnet" else "entropy"
    if args.arithmetic != "f32" and args.model != "enet":
        raise SystemExit("--arithmetic bf16x3 exists for ENet only")
    leg = Leg(args, ctx, args.model, args.classes, c, args.measure, args.weights_seed, args.input_dtype, arithmetic=args.arithmetic)
    model_name = "ICNet" if args.model == "icnet" else "ENet"

    # every rank derives the SAME step counts from the common padded shard length (ceil(POOL / world) frames):
    # shards differ by at most one frame, but ceil(len / batch) of the long and the short shard can differ
    per_rank = (POOL + world - 1) // world
    strong_steps = (per_rank + bs - 1) // bs
    requested_steps, warmup = args.steps, args.warmup
    # the headline region; with --full and N > 1 the other scaling mode is timed beside it
    time_strong = scaling == "strong" or (world > 1 and args.full)
    time_weak = scaling == "weak" or (world > 1 and args.full)
    need = max(strong_steps if time_strong else 0, args.steps + warmup)
    n_resident = leg.make_resident(need)
    log("%d resident batches of %d frames (%.1f GiB) generated on device" %
        (n_resident, bs, n_resident * leg.bytes_per_batch / 2 ** 30))

    # ---- warm-up (untimed) ------------------------------------------------------------------------
    with Watchdog(args.dist_timeout + 120.0, "warm-up"):
        i0, s0, _ = leg.run_steps(max(warmup, 1), 0)
        leg.merge_and_select(i0, s0, max(warmup, 1))
        torch.cuda.synchronize()
    log("warm-up done")

    # ---- timed regions ----------------------------------------------------------------------------
    weak = strong = None
    if time_strong:
        # total work fixed: each rank scores its whole shard of the 2975-frame pool once (a short shard's missing
        # last batch wraps onto batch 0 so that every rank issues the same number of steps; the duplicate is
        # dropped by the scatter-by-index, which writes the same bits twice)
        strong = leg.timed(strong_steps, 0, "strong (pool / %d ranks)" % world)
    if time_weak:
        weak = leg.timed(requested_steps, warmup, "weak (%d steps per rank)" % requested_steps)
    head = strong if scaling == "strong" else weak

    result = None
    if rank == 0:
        frames_head = float(POOL) if scaling == "strong" else head["frames"]
        value = frames_head / head["elapsed"]
        metric = "unlabelled-pool images/sec scored (%s, %dx%d)" % (model_name, h, w)
        workload = "%s pool of %d synthetic %dx%dx%d frames, %s acquisition, batch %d, K=%d, top-%d select%s" % (
            ("configs[3]: ICNet multi-scale (1/4, 1/2, 1; %s)" % ICNET_NOTE) if args.model == "icnet"
            else "configs[1]: ENet", POOL, h, w, c, args.measure, bs, args.classes, TOP_K,
            ", uint8 resident frames" if args.input_dtype == "u8" else "")
        if args.model == "icnet":
            metric += " [%s]" % ICNET_NOTE
        if args.arithmetic != "f32":
            metric += " [OPT-IN arithmetic %s: NOT the reference's arithmetic, not the headline]" % args.arithmetic
            workload += ", arithmetic=%s (opt-in)" % args.arithmetic
        result = {
            "metric": metric, "value": value, "unit": "images/s", "n_gpus": world, "steps": head["steps"],
            "warmup": warmup, "ms_per_step": 1e3 * head["elapsed"] / head["steps"],
            "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
            "dtype": "f32" if args.arithmetic == "f32" else "f32 via bf16x3 (6 products, fp32 accumulate)", "data": "synthetic",
            "config": {"workload": workload, "frames_scored": int(frames_head),
                       "resident_batches_per_rank": n_resident,
                       "sharding": "strided pool shard per rank, one all-gather of (index, score)"},
            "requested_steps": requested_steps,
            "knobs": knobs,
        }
        if world > 1 and args.full:
            other = weak if scaling == "strong" else strong
            oname = "weak" if scaling == "strong" else "strong"
            oframes = other["frames"] if oname == "weak" else float(POOL)
            result[oname] = {"value": oframes / other["elapsed"], "unit": "images/s", "steps": other["steps"],
                             "ms_per_step": 1e3 * other["elapsed"] / other["steps"], "frames_scored": int(oframes),
                             "scaling": oname}
        if args.full:
            # result check: digest of the scores of the frames the timed region scored vs the committed table
            result["score_digest"] = score_digest(head["index"], head["score"], leg.key())
            if args.arithmetic != "f32":  # the mode's own gate: within 1e-6 of the exact table (tests/test_gpu_bf16x3.py)
                dg = result["score_digest"]
                dg["tolerance"] = 1e-6
                dg["bit_identical_to_table"] = bool(dg["sha256"] == dg["expected_sha256"])
                dg["match"] = bool(dg.get("max_abs_diff") is not None and dg["max_abs_diff"] <= 1e-6)
        whole_pool = len(np.unique(head["index"][head["index"] >= 0])) >= POOL
        result["top_k_checksum"] = int(np.sort(head["low"]).astype(np.int64).sum()) if whole_pool else None
        if args.dump_outputs:
            dump_outputs(head, args.dump_outputs)

    # ---- roofline leg: per-kernel HIP-event timing of extra batches (rank 0, outside the clock) ----
    if rank == 0 and args.full and not args.no_roofline:
        result["roofline"], result["roofline_all"] = roofline_leg(leg.net, leg.batches[0][0], args.measure, args.model,
                                                                  arithmetic=args.arithmetic)
        log("roofline leg done")

    # ---- the other single-GPU BASELINE configs (rank 0, N = 1 only) ---------------------------------
    if rank == 0 and world == 1 and args.full and not args.no_secondary and args.model == "enet" and (h, w) == (1024, 2048):
        leg.batches = leg.batches[:1]  # free the resident pool shard (keeps the roofline batch)
        torch.cuda.empty_cache()
        result["secondary"] = {
            "c4": secondary_leg(args, ctx, "c4", "icnet", 19, 3, "margin", 0,
                                "configs[3]: ICNet multi-scale (1/4, 1/2, 1), 1024x2048x3, K=19, margin; " + ICNET_NOTE),
            "c5": secondary_leg(args, ctx, "c5", "enet", 6, 4, "entropy", 1,
                                "configs[4]: ENet Freiburg-Forest shaped (RGB+NIR, 4-channel input), 1024x2048x4, K=6, "
                                "entropy"),
            # OPT-IN arithmetic, never the headline: the headline line, its dtype and its score_digest stay on the exact kernels
            "c2_bf16x3": secondary_leg(args, ctx, "c2_bf16x3", "enet", 19, 3, "entropy", 0,
                                       "configs[1] workload in the OPT-IN arithmetic mode bf16x3 (ENet.score(arithmetic="
                                       "'bf16x3'): the sixteen 128-channel bottlenecks + Bottleneck2_0 / 4_0 on split-operand bf16 MFMAs; NOT the "
                                       "reference's arithmetic, within north_star's 1e-4 / identical top-k: tests/test_gpu_bf16x3.py)",
                                       arithmetic="bf16x3"),
        }
        log("secondary legs done")

    # ---- CPU baseline leg (rank 0, N=1 only) ------------------------------------------------------
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        P = syn.enet_params_dict(leg.net)
        c1 = None
        if args.model == "enet":
            net1 = ssal.ENet(19)
            net1.build((None, None, None, 3))
            syn.randomize_enet(net1, seed=0)
            c1 = (syn.enet_params_dict(net1), 19)
        result["cpu_baseline"] = cpu_baseline(P, h, w, c, args.measure, args.cpu_seconds, c1=c1, model=args.model)
        result["speedup_vs_cpu_baseline"] = result["value"] / result["cpu_baseline"]["value"]

    rc = 0
    if rank == 0:
        bad = []
        if args.full:
            digests = [("headline", result["score_digest"])]
            for nm, sec in result.get("secondary", {}).items():
                digests.append((nm, sec["score_digest"]))
            bad = [nm for nm, dg in digests if dg["match"] is False]
            result["score_digest_verdict"] = ("MISMATCH: " + ", ".join(bad)) if bad else (
                "ok" if all(dg["match"] for _, dg in digests) else "ok (no committed table entry for: %s)"
                % ", ".join(nm for nm, dg in digests if dg["match"] is None))
        detail_path = args.detail_file or (DETAIL_FILE if args.full else None)
        detail = write_detail(result, detail_path) if detail_path else None
        print(json.dumps(result) if args.full_line else compact_line(result, detail), flush=True)
        if bad and not args.allow_digest_mismatch:
            log("score digest MISMATCH (%s): the timed kernels did not produce the committed scores" % ", ".join(bad))
            rc = 4
    if use_dist:
        with Watchdog(args.dist_timeout, "final barrier"):
            dist.barrier()
            dist.destroy_process_group()
    return rc


if __name__ == "__main__":
    sys.exit(main())
