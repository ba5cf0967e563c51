#!/usr/bin/env python
"""The GPU inflater for ordinary gzip input by itself (tbk_gzip_inflate_bench_device): one member of FASTQ made here, `--reps` passes
over it at each of the chunk sizes given.  One JSON line per chunk size: GB/s of text for the kernels alone (marker inflate; propagate +
resolve + CRC-32) and through the whole loop as tbk_gzip_inflate_device drives it, the host's seconds of block-start guessing per GB of
input, chunks accepted / guessed.  `rocprofv3 --kernel-trace --stats -- python tools/measure_gzinflate.py ...` splits the passes."""
import argparse
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--mb", type=int, default=256, help="MB of FASTQ text")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--level", type=int, default=6)
ap.add_argument("--read-len", type=int, default=15000)
ap.add_argument("--chunks", default="65536,131072,262144", help="compressed bytes per chunk, comma separated")
ap.add_argument("--window", type=int, default=0, help="compressed bytes per window (0: the default)")
ap.add_argument("--device", type=int, default=0)
a = ap.parse_args()

from trio_binning_amd import seq  # noqa: E402
from trio_binning_amd._lib import check, lib  # noqa: E402

rng = np.random.default_rng(1)
L = a.read_len
n_reads = max(1, a.mb * 1_000_000 // (2 * L + 40))
recs = []
for i in range(n_reads):
    qv = np.clip(rng.normal(60, 15, L), 2, 93).astype(np.uint8)
    qv[rng.random(L) < 0.6] = 93
    recs.append(b"@read%d/ccs\n" % i + np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, L)].tobytes() + b"\n+\n" + (qv + 33).tobytes() + b"\n")
text = b"".join(recs)
co = zlib.compressobj(a.level, zlib.DEFLATED, 31)
data = co.compress(text) + co.flush()
del recs
for chunk in (int(c) for c in a.chunks.split(",")):
    os.environ["TBK_GZIP_CHUNK"] = str(chunk)
    if a.window:
        os.environ["TBK_GZIP_WINDOW"] = str(a.window)
    assert seq.gzip_inflate_device(data, a.device) == text
    st = seq.gzip_inflate_stats()
    ring, kern, n = C.c_double(), C.c_double(), C.c_uint64()
    passes = (C.c_double * 3)()
    check(lib.tbk_gzip_inflate_bench_device(a.device, data, len(data), a.reps, C.byref(ring), C.byref(kern), C.byref(n), passes))
    gb = n.value / 1e9
    print(json.dumps({"text_GB": round(gb, 3), "file_GB": round(len(data) / 1e9, 3), "level": a.level, "chunk": chunk, "window": a.window or "default",
                      "kernels_GB_per_s": round(gb / kern.value, 2), "ring_GB_per_s": round(gb / ring.value, 2),
                      "marker_inflate_GB_per_s": round(gb / passes[0], 2), "propagate_resolve_crc_GB_per_s": round(gb / passes[1], 2),
                      "guess_s_per_GB_of_input": round(passes[2] / (len(data) / 1e9), 3), "guess_s": round(passes[2], 4), "ring_s": round(ring.value, 4),
                      "kernels_s": round(kern.value, 4), **st}), flush=True)
