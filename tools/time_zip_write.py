"""Timing of the ZIP writer: chip_zip_write as a whole; its parts alone in the same process on the same box -- chip_encode_batch(
CHIP_FMT_DEFLATE, level) over the same units (the yardstick), chip_crc32_batch over the contents, chip_zip_assemble from those streams
and CRCs in both copy shapes (one launch with a source selector per unit; one launch per source buffer, CHIP_ZIPW_COPY=launches) --
and one chip_pack_units of the encoded streams, the plain copy of about the same bytes:
python tools/time_zip_write.py [entries] [content KiB per entry] [repeats] [level]
`entries` (default 16384) entries of `content KiB` (default 64) of the bench payload generator (bench_support.synth) each, all asking
for method 8, level 6.  After two warm-up rounds, `repeats` (default 10) rounds of every measurement, alternating, each timed with
device events (the writer's calls are synchronous, so their window is the whole call: kernels, the waits and the host work between
them).  Prints the median and the fastest of each, the writer's cost over the bare encode as a ratio, and the assembly against
CRC pass + pack; checks the archive with zipfile (a sample of entries) and the two copy shapes against each other."""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import compu_amd  # noqa: E402
from bench_support import synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
ENTRY = (int(sys.argv[2]) if len(sys.argv) > 2 else 64) * 1024
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
level = int(sys.argv[4]) if len(sys.argv) > 4 else 6
threads = min(16, len(os.sched_getaffinity(0)))
dev = torch.device("cuda:0")

pay = synth.payloads(n * ENTRY // synth.UNIT, threads=threads) if ENTRY >= synth.UNIT else synth.payloads(n, unit_size=ENTRY, threads=threads)
src = np.zeros(n, compu_amd.zip_source_dtype())
src["data_off"], src["size"] = np.arange(n, dtype=np.uint64) * ENTRY, ENTRY
src["name_off"], src["name_len"], src["method"], src["dos_date"] = np.arange(n, dtype=np.uint64) * 8, 8, 8, 0x21
names = b"".join(b"e%07d" % k for k in range(n))
d_src = torch.from_numpy(src.view(np.uint8).reshape(-1, 32).copy()).to(dev)
d_names = torch.from_numpy(np.frombuffer(names, np.uint8).copy()).to(dev)
d_content = torch.from_numpy(np.ascontiguousarray(pay)).to(dev)
slot = (compu_amd.encode_bound(-15, ENTRY) + 15) // 16 * 16
d_area = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
in_off = torch.arange(n, dtype=torch.int64, device=dev) * ENTRY
in_len = torch.full((n,), ENTRY, dtype=torch.int32, device=dev)
len64 = torch.full((n,), ENTRY, dtype=torch.int64, device=dev)
slot_off = torch.arange(n, dtype=torch.int64, device=dev) * slot
slot_cap = torch.full((n,), slot, dtype=torch.int32, device=dev)
room = compu_amd.zip_write_bound(n, len(names), n * ENTRY)
d_out = torch.zeros(room, dtype=torch.uint8, device=dev)
d_out2 = torch.zeros(room, dtype=torch.uint8, device=dev)
d_packed = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
state = {}


def write():
    state["write"] = compu_amd.zip_write(d_src, d_names, d_content, level=level, out=d_out)


def encode():
    state["enc"] = compu_amd.encode_batch(-15, level, d_content, in_off, in_len, d_area, slot_off, slot_cap)


def crc_pass():
    state["crc"] = compu_amd.crc32_batch(d_content, in_off, len64)


def assemble(shape):
    def run():
        if shape:
            os.environ["CHIP_ZIPW_COPY"] = shape
        else:
            os.environ.pop("CHIP_ZIPW_COPY", None)
        out_len, _ = state["enc"]
        state["asm" + shape] = compu_amd.zip_assemble(d_src, d_names, d_content, state["crc"], d_area, slot_off, out_len, out=d_out2)
        os.environ.pop("CHIP_ZIPW_COPY", None)

    return run


def pack():
    out_len, _ = state["enc"]
    state["pack"] = compu_amd.pack_units(d_area, slot_off, out_len, d_packed)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


steps = [("zip_write", write), ("encode alone", encode), ("crc alone", crc_pass), ("assemble, one launch", assemble("")),
         ("assemble, launch per source", assemble("launches")), ("pack_units of the streams", pack)]
for _ in range(2):
    for _, fn in steps:
        fn()
torch.cuda.synchronize()
times = {name: [] for name, _ in steps}
for _ in range(reps):
    for name, fn in steps:
        times[name].append(timed(fn))
archive, entries, summ = state["write"]
a1, _, s1 = state["asm"]
a2, _, s2 = state["asmlaunches"]
same_shapes = s1.as_tuple() == s2.as_tuple() == summ.as_tuple() and bool(torch.equal(a1, archive))
d_out2.zero_()
assemble("launches")()
same_shapes = same_shapes and bool(torch.equal(state["asmlaunches"][0], archive))
host = archive.cpu().numpy().tobytes()
zf = zipfile.ZipFile(io.BytesIO(host))
infos = zf.infolist()
sample = sorted({0, 1, n // 3, n // 2, n - 1})
readable = len(infos) == n and all(np.array_equal(np.frombuffer(zf.open(infos[k]).read(), np.uint8), pay[k * ENTRY:(k + 1) * ENTRY]) for k in sample)
med = {k: float(np.median(v)) for k, v in times.items()}
gib = n * ENTRY / 2**30
parts = ", ".join(f"{k} {med[k]:.3f} ms (min {min(times[k]):.3f})" for k, _ in steps)
asm = med["assemble, one launch"]
print(f"zip write {n} entries x {ENTRY} B at level {level} -> {summ.out_len} bytes, {summ.n_deflated} deflated, {reps} rounds: {parts}; "
      f"zip_write {gib / med['zip_write'] * 1e3:.2f} GiB/s in, encode alone {gib / med['encode alone'] * 1e3:.2f} GiB/s in; "
      f"zip_write / encode {med['zip_write'] / med['encode alone']:.3f}, assemble / (crc + pack) "
      f"{asm / (med['crc alone'] + med['pack_units of the streams']):.3f}, assemble launch-per-source / one launch "
      f"{med['assemble, launch per source'] / asm:.3f} (zipfile reads {len(sample)} sampled entries: {readable}, both copy shapes give the archive: "
      f"{same_shapes})", flush=True)
