"""Cost of the depth encoder (lrl/vision.py) per call: the native path (csrc/lrl_vision.hip) against the torch form of
the same module on the same GPU.

At each batch size (4096 and 16384 images of 48 x 64 by default; 42 extra columns, 187 outputs, hidden 128 — the
distiller's shape) ``forward`` and ``forward_backward`` are timed with HIP events in alternating blocks of ``--calls``
calls, native then torch, ``--blocks`` times in one process; the first block of each is a warm-up and is dropped.  One
JSON line per (batch, direction) with every block's ms per call and the medians.

  python scripts/vision_timing.py [--batches 4096,16384] [--calls 10] [--blocks 5] [--out profiles/vision_encoder_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rapid-locomotion-rl_amd"))

import torch  # noqa: E402
from torch.nn import functional as F  # noqa: E402

from lrl import vision  # noqa: E402


def events_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def measure(batch, calls, blocks, dev, h=48, w=64, extra=42, out=187, hidden=128):
    torch.manual_seed(0)
    enc = vision.DepthEncoder(h, w, out, extra_dim=extra, hidden=hidden).to(dev)
    img = torch.rand(batch, h, w, device=dev) * 3.0
    ex, tg = torch.randn(batch, extra, device=dev), torch.randn(batch, out, device=dev)

    def torch_forward():
        with torch.no_grad():
            return enc(img, ex)

    def torch_forward_backward():
        enc.zero_grad()
        F.mse_loss(enc(img, ex), tg).backward()

    legs = {"forward": (lambda: enc.forward_native(img, ex), torch_forward),
            "forward_backward": (lambda: enc.mse_backward_native(img, ex, tg), torch_forward_backward)}
    rows = []
    for name, (native, torch_form) in legs.items():
        ms = {"native": [], "torch": []}
        for _ in range(blocks + 1):  # alternating blocks; block 0 warms both up
            ms["native"].append(events_ms(native, calls))
            ms["torch"].append(events_ms(torch_form, calls))
        r = {"direction": name, "batch": batch, "height": h, "width": w, "extra": extra, "out": out, "hidden": hidden,
             "calls_per_block": calls, "blocks": blocks}
        for k, v in ms.items():
            r[k + "_ms_blocks"] = [round(x, 4) for x in v[1:]]
            r[k + "_ms"] = round(statistics.median(v[1:]), 4)
        r["native_over_torch"] = round(r["native_ms"] / r["torch_ms"], 3)
        rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,16384")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for batch in (int(b) for b in a.batches.split(",")):
        for r in measure(batch, a.calls, a.blocks, "cuda:0"):
            line = json.dumps(r)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
