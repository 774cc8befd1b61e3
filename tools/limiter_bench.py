#!/usr/bin/env python3
"""Time the look-ahead limiter against the packed 48 kHz stereo decode, the
resample stage and apply_gain.

At one shape (default the C3 shape, 65 536 streams x 32 frames, 44.1 kHz
joint stereo) and with device pointers throughout, one handle and one batch
measure per step
  packed          decode_packed, 44.1 -> 48 kHz stereo (the yardstick)
  packed_limit    decode_packed, then limit on its out and counts (float32)
  decode_limited  decode_limited: the same through handle-owned samples
  limit_f32       limit alone on the packed out, float32 to float32
  limit_i16       limit alone, float32 to int16
  apply_f32       apply_gain alone, float32 to float32: it moves the same
                  bytes and is the floor of the stage
and the device time of the limiter stage (limiter_time_us) next to the
resample stage (resample_time_us).  The variants alternate in rounds inside
one process; every step is timed by device events on the call's stream.  No
call flushes: in the steady state a call emits as many samples as it is fed.
--gain is the pre-gain (default 4: the limiter acts on every stream; its work
does not depend on the data except for one division per index over the
ceiling).  The stage reads 4 bytes and writes 4 or 2 per sample and channel;
a tile of 4096 indices also reads its halo of 1931 frames again, from L2.

Then one long stream: the limiter on the device output of decode_long_packed
(20 000 generated frames to 48 kHz stereo, as tools/normalize_bench.py), n = 1,
flushed, by the host clock around the synchronous calls, against that call's
own time.  Prints one JSON line (and writes it to --out).

  python tools/limiter_bench.py --out profiles/limiter.json
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

HBM_MEASURED = 6.29e12  # float4 copy, bytes/s
HZ, CH = 48000, 2
VARIANTS = ("packed", "packed_limit", "decode_limited", "limit_f32", "limit_i16", "apply_f32")


def med(v):
    return float(np.median(np.array(v)))


def batch_part(a, torch, _gen, mp3_amd):
    n, F = a.streams, a.frames
    buf, offs, sizes = _gen.batch(_gen.C3, 3_000_017, n, F, threads=16)
    d_in = torch.from_numpy(buf).cuda()
    dec = mp3_amd.BatchDecoder(n, F)
    dec.set_timing(True)
    dec.set_output(HZ, CH)
    dec.set_limiter(True, a.ceiling)
    strm = torch.cuda.Stream()
    infos = torch.zeros((n, F, 6), dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    oc = torch.zeros(n, dtype=torch.int32, device="cuda")
    S = mp3_amd.packed_max_samples(HZ, F, 44100)
    SO = mp3_amd.limiter_max_samples(HZ, S)
    out = torch.empty((n, S, CH), dtype=torch.float32, device="cuda")
    scaled = torch.empty_like(out)
    lim = torch.empty((n, SO, CH), dtype=torch.float32, device="cuda")
    lim16 = torch.empty((n, SO, CH), dtype=torch.int16, device="cuda")
    gain = torch.full((n,), a.gain, dtype=torch.float32, device="cuda")
    gr = torch.ones(n, dtype=torch.float32, device="cuda")
    times = {k: [] for k in VARIANTS}
    stage = {k: {"resample": [], "limiter": []} for k in VARIANTS}
    fed = {}
    per = max(1, a.steps // a.rounds)

    def step(k):
        if k == "decode_limited":
            dec.decode_limited(d_in, offs, sizes, F, gain=gain, out=lim, counts=oc, gr=gr, infos=infos,
                               stream=strm.cuda_stream)
        elif k == "limit_f32":
            dec.limit(out, counts, gain, out=lim, out_counts=oc, gr=gr, stream=strm.cuda_stream)
        elif k == "limit_i16":
            dec.limit(out, counts, gain, out=lim16, out_counts=oc, gr=gr, f32=False, stream=strm.cuda_stream)
        elif k == "apply_f32":
            dec.apply_gain(out, counts, gain, out=scaled, stream=strm.cuda_stream)
        else:
            dec.decode_packed(d_in, offs, sizes, F, out=out, counts=counts, infos=infos, stream=strm.cuda_stream)
            if k == "packed_limit":
                dec.limit(out, counts, gain, out=lim, out_counts=oc, gr=gr, stream=strm.cuda_stream)

    for _ in range(a.rounds):
        for k in VARIANTS:
            for i in range(a.warmup + per):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(strm)
                step(k)
                e1.record(strm)
                e1.synchronize()
                if i >= a.warmup:
                    times[k].append(e0.elapsed_time(e1) * 1e3)
                    if k in ("packed", "packed_limit", "decode_limited"):
                        stage[k]["resample"].append(dec.resample_time_us())
                    if k not in ("packed", "apply_f32"):
                        stage[k]["limiter"].append(dec.limiter_time_us())
            print("%s: %.0f us" % (k, med(times[k])), file=sys.stderr, flush=True)
            if k == "packed_limit":
                fed["samples"] = int(counts.cpu().numpy().astype(np.int64).sum())
                g = gr.cpu().numpy()
                fed["gr"] = [float(g.min()), float(g.mean()), float((g < 1.0).mean())]
    res = {"shape": [n, F], "format": [HZ, CH], "steps": len(times["packed"]), "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "unit": "us", "samples_per_call": fed["samples"],
           "ceiling_db": a.ceiling, "pre_gain": a.gain, "gr_min_mean_share_limited": fed["gr"]}
    base = med(times["packed"])
    samples = fed["samples"]  # steady state: every call feeds a call's inputs' worth of samples
    for k in VARIANTS:
        t = np.array(times[k])
        r = res[k] = {"step_median": float(np.median(t)), "step_min": float(t.min()), "step_max": float(t.max()),
                      "step_over_packed": float(np.median(t) / base)}
        if stage[k]["resample"]:
            r["resample_stage_median"] = med(stage[k]["resample"])
        if k == "apply_f32":
            byts = samples * CH * 8
            r.update({"bytes_per_s": byts / (np.median(t) * 1e-6),
                      "share_of_measured_hbm": byts / (np.median(t) * 1e-6) / HBM_MEASURED})
        if stage[k]["limiter"]:
            lt = med(stage[k]["limiter"])
            byts = samples * CH * (4 + (2 if k == "limit_i16" else 4))
            r.update({"limiter_stage_median": lt, "limiter_stage_min": float(np.min(stage[k]["limiter"])),
                      "limiter_stage_share_of_step": lt / float(np.median(t)),
                      "limiter_stage_ns_per_sample": lt * 1e3 / max(samples, 1),
                      "limiter_stage_bytes_per_s": byts / (lt * 1e-6),
                      "limiter_stage_share_of_measured_hbm": byts / (lt * 1e-6) / HBM_MEASURED})
            if "resample_stage_median" in r:
                r["limiter_stage_over_resample_stage"] = lt / r["resample_stage_median"]
    for k in ("limit_f32", "limit_i16", "packed_limit", "decode_limited"):
        res[k]["limiter_stage_over_apply_f32"] = res[k]["limiter_stage_median"] / res["apply_f32"]["step_median"]
    res["decode_limited"]["step_over_packed_limit"] = (res["decode_limited"]["step_median"]
                                                       / res["packed_limit"]["step_median"])
    return res


def long_part(a, torch, _gen, mp3_amd):
    data, _ = _gen.stream(_gen.C3, 3_000_017, a.long_frames)
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    dec = mp3_amd.BatchDecoder(1024, 32 + 11)
    dec.set_timing(True)
    dec.set_output(HZ, CH)
    dec.set_limiter(True, a.ceiling)
    bound = mp3_amd.long_packed_bound(data, HZ)
    out = torch.empty((bound, CH), dtype=torch.float32, device="cuda")
    lim = torch.empty((1, mp3_amd.limiter_max_samples(HZ, bound), CH), dtype=torch.float32, device="cuda")
    oc = torch.zeros(1, dtype=torch.int32, device="cuda")
    gr = torch.ones(1, dtype=torch.float32, device="cuda")
    gain = torch.full((1,), a.gain, dtype=torch.float32, device="cuda")
    t_long, t_call, t_stage = [], [], []
    n = 0
    for i in range(a.warmup + a.long_steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = dec.decode_long_packed(d_in, HZ, CH, segment_frames=32, out=out, gapless=True)
        t1 = time.perf_counter()
        n = int(len(r[0]))
        cnt = torch.tensor([n], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        dec.limit(out[None], cnt, gain, out=lim, out_counts=oc, gr=gr, flush=True)
        dec.sync()
        t3 = time.perf_counter()
        if i >= a.warmup:
            t_long.append((t1 - t0) * 1e6)
            t_call.append((t3 - t2) * 1e6)
            t_stage.append(dec.limiter_time_us())
    assert int(oc.cpu()[0]) == n
    return {"frames": a.long_frames, "out_samples": n, "gr": float(gr.cpu()[0]),
            "decode_long_packed_call_median": med(t_long), "limit_call_median": med(t_call),
            "limit_stage_median": med(t_stage), "limit_call_over_decode_long_packed": med(t_call) / med(t_long),
            "limit_stage_ns_per_sample": med(t_stage) * 1e3 / max(n, 1),
            "limit_stage_bytes_per_s": n * CH * 8 / (med(t_stage) * 1e-6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--gain", type=float, default=4.0)
    ap.add_argument("--ceiling", type=float, default=-1.0)
    ap.add_argument("--long-frames", type=int, default=20000)
    ap.add_argument("--long-steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import _gen
    import mp3_amd

    assert torch.cuda.is_available(), "needs an MI355X"
    res = batch_part(a, torch, _gen, mp3_amd)
    res["long"] = long_part(a, torch, _gen, mp3_amd)
    print(json.dumps(res))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
