"""SURVEY config 4 ("all 11 EuRoC sequences batched"), on synthetic streams of
the same shape (EuRoC is not reachable here): S stereo+IMU sequences replayed
through ONE device context by the multi-sequence scheduler
(msckf_amd.scheduler.MultiMSCKF), against the same S sequences replayed one
after another through the single-filter drop-in class.  Prints one JSON line:
frames/s of both, the batched launch counts, and ATE vs ground truth.  The
replayed messages (the front-end's output) are built before both timed
regions.

    python tools/bench_sequences.py [--seqs 11] [--frames 200] [--fp32] [--device-map [--device-keyframes]]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 \
        tools/bench_sequences.py --seqs 11      # sequences dealt round-robin over N GPUs

--device-map keeps the lanes' feature maps on the device (msckf_map.h) and
feeds the frames as array messages (msckf.FeatureArrays); --device-keyframes
(with --device-map) chooses a prune frame's cam states on the device
(msckf_keyframes.h); --profile prints a cProfile split of the batched replay to
stderr.  --landmarks {host,device} keeps the landmark archive and --odometry
reads the pose covariance with every frame (msckf_odometry.h); --kernel-times
adds the stage times of a second, untimed replay.  --zupt turns the
zero-velocity update on with the default ZuptConfig (msckf_zupt.h; its kernels
are zupt_gain and zupt_apply in --kernel-times) and reports how many updates
the device applied; --static-s S is the streams' time at rest before they move
(synth.make_sequence's static_s).  --aiding turns the aiding fixes on
(msckf_aid.h; kernels aid_gain and aid_apply): position + velocity messages
from the streams' ground truth at --aid-rate Hz (default 5), 12 ms before a
frame, with 2 cm / 2 cm/s noise, rotated into each filter's world frame, and
reports how many fixes the device applied.  --aid-latency S (with --aiding)
hands every fix over S seconds after its stamp (AidingFix.received) and turns
AidingConfig.delayed on: the fixes older than max_age take the delayed path on
the window's clones (msckf_aid_delayed.h; kernels aid_delayed_gain and
aid_delayed_apply; their velocity rows are left out), and the line reports how
many of them the device applied.  --anchors turns the anchor fixes on
(msckf_anchor.h; kernels anchor_gain and anchor_apply): --anchor-n (default 8)
points per stream surveyed to 5 mm, their stereo observations from the ground
truth with the streams' pixel noise at --anchor-rate Hz (default 5), at the
frame times, and reports how many updates the device applied.

On N GPUs every rank replays its share of the sequences (replicas.shard) on
its own device; the replicas' host TCP hub (msckf_amd.replicas, no RCCL:
no data crosses GPUs) carries only the barriers, the max of the elapsed time
and the sum of the frame counts (SURVEY config 4: no cross-GPU state).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import msckf_pkg  # noqa: E402,F401
import msckf_amd  # noqa: E402
from msckf_amd import synth, replicas  # noqa: E402
from msckf_amd.replay import FeatureStream, replay  # noqa: E402
from msckf_amd.scheduler import MultiMSCKF  # noqa: E402
from msckf_amd.trajectory import ate  # noqa: E402


def aiding_fixes(seq, static_s, rate, seed, lead=0.012, sigma=0.02, t_start=100.0, latency=None):
    """Position + velocity messages for ``seq`` from its ground truth, in the
    filter's world frame: ``lead`` before every (20 / rate)-th frame from the
    first one the filter publishes (one second of gravity initialisation), with
    ``sigma`` noise.  The two world frames are aligned by A = R_filter_iw
    R_truth_iw^T at that frame, where both origins are 0 (the stream rests): the
    filter's initial attitude is the one its gravity initialisation will
    compute from the first 200 IMU samples.  ``latency``: the messages reach the
    filter that many seconds after their stamp."""
    A, first = _alignment(seq)
    rng = np.random.default_rng(seed)
    t0, h, out = t_start + static_s, 1e-4, []
    for k in range(first, len(seq.gt_t), max(1, int(round(20.0 / rate)))):
        t = seq.gt_t[k] - lead
        p = synth._traj(t, t0)[0]
        v = (synth._traj(t + h, t0)[0] - synth._traj(t - h, t0)[0]) / (2 * h)
        out.append(msckf_amd.AidingFix(t, position=A @ p + sigma * rng.standard_normal(3),
                                       velocity=A @ v + sigma * rng.standard_normal(3),
                                       position_var=sigma ** 2, velocity_var=sigma ** 2,
                                       received=None if latency is None else t + latency))
    return out


def _alignment(seq):
    """(A, first): A rotates the synthetic world into the filter's (aiding_fixes), first the first published frame."""
    from msckf_amd.geometry import from_two_vectors, to_rotation
    g_imu = np.mean([m.linear_acceleration for m in seq.imu[:200]], axis=0)
    q0 = from_two_vectors(-np.array([0.0, 0.0, -np.linalg.norm(g_imu)]), g_imu)
    first = int(np.searchsorted(seq.gt_t, seq.imu[199].vio_timestamp__))
    return to_rotation(q0).T @ seq.gt_R[first].T, first


def anchor_fixes(seq, rate, n, seed, sigma=0.005, pix_sigma=0.5 / 458.654):
    """Anchor messages for ``seq`` from its ground truth: ``n`` points uniform
    in the box [4, -2.5, -1.5] .. [7, 2.5, 1.5] of the synthetic world, given in
    the filter's world frame (aligned as in ``aiding_fixes``) with ``sigma``
    survey noise and declared so; a message AT every (20 / rate)-th frame from
    the first one the filter publishes with the points that pass
    make_sequence's visibility test, their true projections plus ``pix_sigma``
    noise."""
    cfg = msckf_amd.FilterConfig()
    R_ic, t_ic = cfg.T_imu_cam0[:3, :3], cfg.T_imu_cam0[:3, 3]
    Rcc, tcc = cfg.T_cn_cnm1[:3, :3], cfg.T_cn_cnm1[:3, 3]
    A, first = _alignment(seq)
    rng = np.random.default_rng(seed)
    lo, hi = np.array([4.0, -2.5, -1.5]), np.array([7.0, 2.5, 1.5])
    L = lo + (hi - lo) * rng.random((n, 3))
    declared = L @ A.T + sigma * rng.standard_normal((n, 3))
    out = []
    for k in range(first, len(seq.gt_t), max(1, int(round(20.0 / rate)))):
        R0 = R_ic @ seq.gt_R[k].T
        t_c0 = seq.gt_p[k] + seq.gt_R[k] @ (-R_ic.T @ t_ic)
        R1 = Rcc @ R0
        pc0, pc1 = (L - t_c0) @ R0.T, (L - (t_c0 - R1.T @ tcc)) @ R1.T
        with np.errstate(divide="ignore", invalid="ignore"):
            uv = np.stack([pc0[:, 0] / pc0[:, 2], pc0[:, 1] / pc0[:, 2], pc1[:, 0] / pc1[:, 2], pc1[:, 1] / pc1[:, 2]], 1)
        vis = (pc0[:, 2] > 0.5) & (pc1[:, 2] > 0.5) & (np.abs(uv[:, [0, 2]]) < 0.75).all(1) & (np.abs(uv[:, [1, 3]]) < 0.5).all(1)
        idx = np.flatnonzero(vis)
        if len(idx):
            out.append(msckf_amd.AnchorFix(seq.gt_t[k], declared[idx], uv[idx] + pix_sigma * rng.standard_normal((len(idx), 4)),
                                           sigma ** 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=11)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--fp32", action="store_true")
    ap.add_argument("--no-single", action="store_true")
    ap.add_argument("--device-map", action="store_true")
    ap.add_argument("--device-keyframes", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--landmarks", choices=("host", "device"), default=None,
                    help="keep the landmark archive (msckf_odometry.h): in numpy, or on the device (needs --device-map)")
    ap.add_argument("--odometry", action="store_true", help="the frames' reads bring the pose covariance along")
    ap.add_argument("--zupt", action="store_true",
                    help="the zero-velocity update (msckf_zupt.h), default ZuptConfig")
    ap.add_argument("--static-s", type=float, default=None,
                    help="seconds at rest at the start of every stream (make_sequence's static_s; default: its own)")
    ap.add_argument("--aiding", action="store_true",
                    help="aiding fixes (msckf_aid.h): synthetic position + velocity messages from the ground truth")
    ap.add_argument("--aid-rate", type=float, default=5.0, help="fixes per second and stream with --aiding")
    ap.add_argument("--aid-latency", type=float, default=None,
                    help="with --aiding: the fixes arrive this many seconds late and AidingConfig.delayed is on "
                         "(msckf_aid_delayed.h)")
    ap.add_argument("--anchors", action="store_true",
                    help="anchor fixes (msckf_anchor.h): synthetic surveyed points observed from the ground truth")
    ap.add_argument("--anchor-n", type=int, default=8, help="anchors per stream with --anchors")
    ap.add_argument("--anchor-rate", type=float, default=5.0, help="anchor messages per second and stream with --anchors")
    ap.add_argument("--kernel-times", action="store_true",
                    help="a second, untimed batched replay with every stage timed (msckf_kernel_times)")
    a = ap.parse_args()
    if a.device_keyframes and not a.device_map:
        ap.error("--device-keyframes needs --device-map")
    if a.aid_latency is not None and not a.aiding:
        ap.error("--aid-latency needs --aiding")
    if a.landmarks == "device" and not a.device_map:
        ap.error("--landmarks device needs --device-map")
    opt = dict(landmarks=a.landmarks, odometry=a.odometry) if a.landmarks or a.odometry else {}
    if a.zupt:
        opt["zupt"] = msckf_amd.ZuptConfig()
    if a.aiding:
        opt["aiding"] = msckf_amd.AidingConfig(delayed=a.aid_latency is not None)
    if a.anchors:
        opt["anchors"] = msckf_amd.AnchorConfig()
    seq_kw = {} if a.static_s is None else dict(static_s=a.static_s)
    dtype = np.float32 if a.fp32 else np.float64
    grp = replicas.init()
    mine = replicas.shard(list(range(a.seqs)), grp.rank, grp.world)
    seqs = [synth.make_sequence(a.frames, 100 + i, **seq_kw) for i in mine]
    streams = [FeatureStream.from_synthetic(q) for q in seqs]
    fixes = [aiding_fixes(q, 1.2 if a.static_s is None else a.static_s, a.aid_rate, 1000 + i, latency=a.aid_latency)
             for q, i in zip(seqs, mine)] if a.aiding else None
    anchor_msgs = [anchor_fixes(q, a.anchor_rate, a.anchor_n, 2000 + i) for q, i in zip(seqs, mine)] if a.anchors else None
    n_frames = sum(s.n_frames for s in streams)
    multi = MultiMSCKF(len(streams), dtype=dtype, device=grp.local_rank,
                       device_map=a.device_map, device_keyframes=a.device_keyframes, **opt) if streams else None
    # the messages are the front-end's output: built before either timed
    # region (as the bench's ATE leg does), fresh objects for each run
    msgs = [s.messages(arrays=a.device_map) for s in streams]
    if fixes:   # the messages of the aiding sensor are inputs too
        for i, fx in enumerate(fixes):
            for f in fx:
                multi.aiding_callback(i, f)
    for i, fx in enumerate(anchor_msgs or []):
        for f in fx:
            multi.anchor_callback(i, f)
    grp.barrier()
    prof = None
    if a.profile:
        import cProfile
        prof = cProfile.Profile()
        prof.enable()
    t0 = time.perf_counter()
    trajs = multi.run_streams(streams, messages=msgs) if multi else []
    el_b = grp.max_over_ranks(time.perf_counter() - t0)
    if prof is not None:
        import pstats
        prof.disable()
        pstats.Stats(prof, stream=sys.stderr).sort_stats("tottime").print_stats(25)
    total_frames = grp.sum_over_ranks(n_frames)
    launches = dict(multi.launches) if multi else {}
    archived = [int(multi.landmarks(i).next_seq) for i in range(len(streams))] if multi and a.landmarks else None
    zupt_applied = [[int(ln.zupt_count), len(ln.zupt_log)] for ln in multi.lanes] if multi and a.zupt else None
    aid_applied = [[int(ln.aid_count), len(ln.aid_log)] for ln in multi.lanes] if multi and a.aiding else None
    delayed_applied = [[int(ln.aid_delayed_count), len(ln.aid_delayed_log)] for ln in multi.lanes] \
        if multi and a.aid_latency is not None else None
    anchor_applied = [[int(ln.anchor_count), len(ln.anchor_log)] for ln in multi.lanes] if multi and a.anchors else None
    if multi:
        multi.close()
    kernel_ms = None
    if a.kernel_times and streams:   # outside the timed region, on a fresh context: stage times of one replay
        prof_run = MultiMSCKF(len(streams), dtype=dtype, device=grp.local_rank, device_map=a.device_map,
                              device_keyframes=a.device_keyframes, **opt)
        prof_run.ctx.set_profiling(True)
        for i, fx in enumerate(fixes or []):
            for f in fx:
                prof_run.aiding_callback(i, f)
        for i, fx in enumerate(anchor_msgs or []):
            for f in fx:
                prof_run.anchor_callback(i, f)
        prof_run.run_streams(streams, messages=[s.messages(arrays=a.device_map) for s in streams])
        kernel_ms = {k: [round(ms, 3), n] for k, (ms, n) in prof_run.ctx.kernel_times().items()}
        prof_run.close()
    out = {"config": "SURVEY config 4 shape: %d synthetic stereo+IMU sequences x %d frames, %s, %d GPU(s)"
                     % (a.seqs, a.frames, "fp32" if a.fp32 else "fp64", grp.world),
           "batched_frames_per_s": round(total_frames / el_b, 1), "batched_s": round(el_b, 2),
           "device_map": bool(a.device_map), "device_keyframes": bool(a.device_keyframes),
           "batched_launches_rank0": launches,
           "ate_vs_gt_m_rank0": [round(ate(t, s.gt), 5) for t, s in zip(trajs, streams)]}
    if a.landmarks or a.odometry:   # (without the options the line is what it was)
        out.update(landmarks=a.landmarks, odometry=bool(a.odometry))
    if a.static_s is not None:
        out["static_s"] = a.static_s
    if zupt_applied is not None:   # per lane: updates applied, updates enqueued
        out["zupt_applied_of_rank0"] = zupt_applied
    if aid_applied is not None:   # per lane: fixes applied, fixes enqueued
        out["aid_applied_of_rank0"] = aid_applied
    if delayed_applied is not None:   # per lane: late fixes applied, late fixes enqueued
        out["aid_latency_s"] = a.aid_latency
        out["aid_delayed_applied_of_rank0"] = delayed_applied
    if anchor_applied is not None:   # per lane: updates applied, messages enqueued
        out["anchor_applied_of_rank0"] = anchor_applied
    if archived is not None:
        out["landmarks_archived_rank0"] = archived
    if kernel_ms is not None:
        out["kernel_ms_launches_rank0"] = kernel_ms
    if not a.no_single and grp.world == 1:
        evs = [s.events() for s in streams]
        if a.device_map:
            evs = [[(k, m if k == 0 else s.frame_arrays(j)) for (k, m), j in
                    zip(ev, np.cumsum([k for k, _ in ev]) - 1)] for s, ev in zip(streams, evs)]
        t0 = time.perf_counter()
        for i, (s, ev) in enumerate(zip(streams, evs)):
            flt = msckf_amd.MSCKF(dtype=dtype, device_map=a.device_map, device_keyframes=a.device_keyframes, **opt)
            for f in (fixes[i] if fixes else []):
                flt.aiding_callback(f)
            for f in (anchor_msgs[i] if anchor_msgs else []):
                flt.anchor_callback(f)
            replay(flt, s, events=ev)
            flt.close()
        el_s = time.perf_counter() - t0
        out["single_frames_per_s"] = round(n_frames / el_s, 1)
        out["single_s"] = round(el_s, 2)
        out["speedup"] = round(el_s / el_b, 2)
    if grp.rank != 0:
        grp.close()
        return
    print(json.dumps(out), flush=True)
    grp.close()


if __name__ == "__main__":
    main()
