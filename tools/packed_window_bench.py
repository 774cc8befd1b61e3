#!/usr/bin/env python3
"""Time the packed sink's sample windows against the parent commit's library.

At the C3 shape (65 536 streams x 32 frames, 44.1 kHz joint stereo) and with
device pointers throughout, measures decode_packed to 16 kHz mono and to
48 kHz stereo with four variants that alternate in rounds inside one process:
  parent   the parent commit's library (no windows), --parent build_ab/PARENT.so
           from `python abx/build_rev.py PARENT <parent rev>`
  plain    this library, no flag
  gapless  this library, MP3D_PACK_GAPLESS on every call (the generated
           streams carry no tag: the cost of fixing the windows, nothing cut)
  window   this library, the window [1105, no end) set on every slot before
           each step (outside the timed region), so every step skips 1105
           samples per stream inside its first frame
Every step is timed by device events on the call's stream; the resample
stage's own device time is resample_time_us.  Per variant: the median step,
the median stage time, the median of each round and their spread
(max - min) / median.  "plain" is compared with "parent", whose own
round-to-round spread is the allowance; "gapless" and "window" are ratios to
"plain".  Prints one JSON line (and writes it to --out).

  python abx/build_rev.py PARENT HEAD~1
  python tools/packed_window_bench.py --parent build_ab/PARENT.so --out profiles/packed_window.json
"""
import argparse
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

FORMATS = {"16k_mono": (16000, 1), "48k_stereo": (48000, 2)}
VARIANTS = ["parent", "plain", "gapless", "window"]
SKIP = 1105  # the tagged golden's enc_delay + 529


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=str(ROOT / "build_ab" / "PARENT.so"))
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--steps", type=int, default=6, help="timed steps per variant and round")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import _gen
    import mp3_amd

    assert torch.cuda.is_available(), "needs an MI355X"
    n, F = a.streams, a.frames
    buf, offs, sizes = _gen.batch(_gen.C3, 3_000_017, n, F, threads=16)
    d_in = torch.from_numpy(buf).cuda()
    with mp3_amd.library(a.parent):
        old = mp3_amd.BatchDecoder(n, F)
    new = mp3_amd.BatchDecoder(n, F)
    for d in (old, new):
        d.set_timing(True)
    strm = torch.cuda.Stream()
    infos = torch.zeros((n, F, 6), dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    lo = np.full(n, SKIP, np.int64)
    step_us = {f: {v: [[] for _ in range(a.rounds)] for v in VARIANTS} for f in FORMATS}
    stage_us = {f: {v: [] for v in VARIANTS} for f in FORMATS}
    emitted = {f: {} for f in FORMATS}
    for rnd in range(a.rounds):
        for f, fmt in FORMATS.items():
            out = torch.empty((n, mp3_amd.packed_max_samples(fmt[0], F, 44100), fmt[1]), dtype=torch.float32,
                              device="cuda")
            for v in VARIANTS[rnd % len(VARIANTS):] + VARIANTS[:rnd % len(VARIANTS)]:  # each goes first once in four
                dec = old if v == "parent" else new
                dec.reset()
                dec.set_output(*fmt)  # (restarts resamplers and windows)
                kw = {"gapless": True} if v == "gapless" else {}
                for i in range(a.warmup + a.steps):
                    if v == "window":
                        dec.set_window(lo)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(strm)
                    dec.decode_packed(d_in, offs, sizes, F, out=out, counts=counts, infos=infos,
                                      stream=strm.cuda_stream, **kw)
                    e1.record(strm)
                    e1.synchronize()
                    if i >= a.warmup:
                        step_us[f][v][rnd].append(e0.elapsed_time(e1) * 1e3)
                        stage_us[f][v].append(dec.resample_time_us())
                emitted[f][v] = int(counts.cpu().numpy().astype(np.int64).sum())
            del out
    res = {"shape": [n, F], "steps_per_round": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "unit": "us", "window": [SKIP, None]}
    for f in FORMATS:
        r = {}
        for v in VARIANTS:
            per_round = [float(np.median(t)) for t in step_us[f][v]]
            med = float(np.median(np.concatenate(step_us[f][v])))
            r[v] = {"step_median": med, "stage_median": float(np.median(stage_us[f][v])), "round_medians": per_round,
                    "round_spread": (max(per_round) - min(per_round)) / med, "last_call_samples": emitted[f][v]}
        r["plain_over_parent"] = r["plain"]["step_median"] / r["parent"]["step_median"]
        r["plain_over_parent_stage"] = r["plain"]["stage_median"] / r["parent"]["stage_median"]
        r["allowance_parent_round_spread"] = r["parent"]["round_spread"]
        r["gapless_over_plain"] = r["gapless"]["step_median"] / r["plain"]["step_median"]
        r["window_over_plain"] = r["window"]["step_median"] / r["plain"]["step_median"]
        r["gapless_over_plain_stage"] = r["gapless"]["stage_median"] / r["plain"]["stage_median"]
        r["window_over_plain_stage"] = r["window"]["stage_median"] / r["plain"]["stage_median"]
        res[f] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
