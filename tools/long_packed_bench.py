#!/usr/bin/env python3
"""Time decode_long_packed against decode_long on one long stream.

Workload: a generated C3 stream (44.1 kHz joint stereo, 128 kbps) of 20 000
frames, device input and device output, segments of 32 frames on a
1 024-stream handle (625 segments: one chunk).  Measures per call, by the
host clock around the synchronous call,
  long        BatchDecoder.decode_long(f32=True) into [n, 2304] rows: the
              baseline, without any trim, channel map or resampling
  48k_stereo  decode_long_packed to 48 kHz stereo, gapless on
  16k_mono    decode_long_packed to 16 kHz mono, gapless on
and, for the packed variants, the sink stage's own device time
(resample_time_us: plan, filter and carry kernels of the chunk).  The variants
alternate in rounds inside one process.  Recorded: the median of the timed
calls, its ratio to the baseline, the stage's ns per input sample and,
alongside, the batched sink's ns per input sample from
profiles/packed_sink.json.  Prints one JSON line (and writes it to --out).

  python tools/long_packed_bench.py --out profiles/long_packed.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20000)
    ap.add_argument("--segment", type=int, default=32)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import _gen
    import mp3_amd

    assert torch.cuda.is_available(), "needs an MI355X"
    data, _ = _gen.stream(_gen.C3, 3_000_017, a.frames)
    n = len(mp3_amd.long_plan(data, a.segment)[0])
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    dec = mp3_amd.BatchDecoder(a.streams, a.segment + 11)
    dec.set_timing(True)
    rows = torch.empty((n, 2304), dtype=torch.float32, device="cuda")
    infos = torch.zeros((n, 6), dtype=torch.int32, device="cuda")
    variants = {"long": None, "48k_stereo": (48000, 2), "16k_mono": (16000, 1)}
    outs = {k: torch.empty((mp3_amd.long_packed_bound(data, v[0]), v[1]), dtype=torch.float32, device="cuda")
            for k, v in variants.items() if v}
    times = {k: [] for k in variants}
    stage = {k: [] for k in variants if variants[k]}
    samples, in_hz = {}, 0
    per = max(1, a.steps // a.rounds)

    def step(k):
        if variants[k] is None:
            dec.decode_long(d_in, a.segment, max_frames=n, pcm=rows, infos=infos, f32=True)
            return None
        hz, ch = variants[k]
        return dec.decode_long_packed(d_in, hz, ch, segment_frames=a.segment, out=outs[k], gapless=True)

    for _ in range(a.rounds):
        for k, fmt in variants.items():
            for i in range(a.warmup + per):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = step(k)
                t1 = time.perf_counter()
                if i >= a.warmup:
                    times[k].append((t1 - t0) * 1e6)
                    if fmt:
                        stage[k].append(dec.resample_time_us())
                if fmt:
                    samples[k], in_hz = int(len(r[0])), int(r[2])
    n_in = int((infos.cpu().numpy()[:, 5]).astype(np.int64).sum())  # input samples per channel
    res = {"frames": n, "segment_frames": a.segment, "max_streams": a.streams, "steps": len(times["long"]),
           "warmup": a.warmup, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "unit": "us",
           "in_hz": in_hz, "input_samples": n_in}
    batched = {}
    ref = ROOT / "profiles" / "packed_sink.json"
    if ref.exists():
        pk = json.loads(ref.read_text())
        for k in ("48k_stereo", "16k_mono"):
            batched[k] = pk[k]["stage_median"] * 1e3 / (pk["shape"][0] * pk["shape"][1] * 1152)
    base = float(np.median(times["long"]))
    for k, fmt in variants.items():
        t = np.array(times[k])
        r = {"call_median": float(np.median(t)), "call_min": float(t.min()), "call_max": float(t.max())}
        if fmt:
            st = np.array(stage[k])
            r.update({"call_over_long": float(np.median(t) / base), "stage_median": float(np.median(st)),
                      "stage_min": float(st.min()), "stage_ns_per_input_sample": float(np.median(st) * 1e3 / n_in),
                      "batched_sink_ns_per_input_sample": batched.get(k), "out_samples": samples[k]})
        res[k] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
