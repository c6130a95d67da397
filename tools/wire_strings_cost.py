"""What STRING fields cost in the wire decoder (flink_amd/csrc/wire.hip, FWA_FIELD_STRING): decode, string extraction
and key dictionary encode of a C2-shaped, device-resident stream.

Streams (built on the device; 2^24 records, keys uniform over --keys distinct values, one watermark element at the end):
  inline   BinaryRowData rows (VARCHAR user, TIMESTAMP(3) rowtime, BIGINT v), every user 5 bytes (inline in its slot):
           41-byte elements of one size, so the walk speculates as on fixed rows
  var      the same rows with users of 8..40 bytes (length and content functions of the key): 49..81-byte elements,
           sizes differ from record to record, so the walk lists elements by scalar steps
  fixed    Tuple3<Long, Long, Long> StreamRecords with timestamps (37 B, the bench's wire_input shape), as many records
           as make the byte volume of `var`
Numbers per stream, mean of --reps decodes after one warm-up:
  decode_ms / scan_ms   fwa_wire_stats (HIP events on the decoder's stream: scan + compose + resolve + decode; scan alone)
  extract_ms            fwa_wire_strings_of of the user field: device scan of the lengths + gather (host clock around a
                        call that ends in a synchronise)
  encode_ms             KeyDictionary.encode of the extracted strings (host clock, likewise)
  wire GB/s             wire bytes / decode_ms, and that over the 8.0 TB/s HBM peak. This is a whole-decode rate (the
                        wire bytes are read twice, by scan and decode, and the columns written once), not one kernel's
                        share of the peak.
Output: python tools/wire_strings_cost.py > profiles/<tag>_wire_strings_cost.txt"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flink_amd import wire  # noqa: E402
from flink_amd.keydict import KeyDictionary  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--records", type=int, default=1 << 24)
ap.add_argument("--keys", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--streams", default="inline,var,fixed")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("wire_strings_cost.py measures on the GPU: none found")
dev = torch.device("cuda", 0)
HBM_PEAK_GBPS = 8000.0
N = args.records
g = torch.Generator(device=dev)
g.manual_seed(0x5eed)
keys = torch.randint(0, args.keys, (N,), device=dev, generator=g, dtype=torch.int64)
ts = 1_700_000_000_000 + torch.arange(N, device=dev, dtype=torch.int64) // 1000
vals = torch.randint(0, 1 << 31, (N,), device=dev, generator=g, dtype=torch.int64)
WM = torch.tensor([0, 0, 0, 9, 2, 0, 0, 1, 0x8B, 0xCF, 0xE5, 0x68, 0], dtype=torch.uint8, device=dev)   # watermark element


def le(x):   # int64 -> its 8 little-endian bytes per element
    return x.contiguous().view(torch.uint8).view(-1, 8)


def hexchar(j):   # ASCII of hex digit j % 5 of the key: 5 digits tell 2^20 keys apart
    nib = (keys >> (4 * (j % 5))) & 15
    return torch.where(nib < 10, nib + 48, nib + 87).to(torch.uint8)


def inline_stream():
    rec = torch.zeros(N, 41, dtype=torch.uint8, device=dev)
    rec[:, 3], rec[:, 4], rec[:, 8] = 37, 1, 32                  # be32 L | TAG_REC_WITHOUT_TIMESTAMP | be32 size
    for j in range(5):
        rec[:, 17 + j] = hexchar(j)
    rec[:, 24] = 0x85                                            # inline, 5 bytes
    rec[:, 25:33] = le(ts)
    rec[:, 33:41] = le(vals)
    return torch.cat([rec.reshape(-1), WM])


def var_stream():
    ln = 8 + keys % 33
    pad = (ln + 7) & ~7
    esz = 41 + pad
    start = torch.cumsum(esz, 0) - esz
    out = torch.zeros(int(esz.sum().item()) + 13, dtype=torch.uint8, device=dev)
    out[start + 3] = (37 + pad).to(torch.uint8)
    out[start + 4] = 1
    out[start + 8] = (32 + pad).to(torch.uint8)
    out[start + 17] = ln.to(torch.uint8)                         # slot = 32 << 32 | length
    out[start + 21] = 32
    tb, vb = le(ts), le(vals)
    for j in range(8):
        out[start + 25 + j] = tb[:, j]
        out[start + 33 + j] = vb[:, j]
    for j in range(40):
        m = ln > j
        out[(start + 41 + j)[m]] = hexchar(j)[m]
    out[-13:] = WM
    return out


def fixed_stream(nbytes):
    n = min(N * 4, nbytes // 37)
    k, t, v = (x.repeat((n + N - 1) // N)[:n] for x in (keys, ts, vals))

    def be(x):
        return le(x).flip(1)
    rec = torch.zeros(n, 37, dtype=torch.uint8, device=dev)
    rec[:, 3] = 33
    rec[:, 5:13], rec[:, 13:21], rec[:, 21:29], rec[:, 29:37] = be(t), be(k), be(t), be(v)
    return torch.cat([rec.reshape(-1), WM]), n


def run(name, buf, n, schema, strings):
    dec = wire.WireDecoder(schema)
    kd = KeyDictionary(["STRING"], capacity=2 * args.keys) if strings else None
    ext = enc = 0.0
    st0 = None
    for rep in range(args.reps + 1):
        d = dec.decode(buf)
        assert d.n_records == n and d.n_events == 1 and d.consumed == buf.numel()
        if strings:
            t0 = time.perf_counter()
            offs, data, nul = d.strings(0)
            t1 = time.perf_counter()
            kd.encode([(offs, data)], [nul])
            t2 = time.perf_counter()
            if rep:
                ext += t1 - t0
                enc += t2 - t1
        if rep == 0:
            st0 = dec.stats()
    st = dec.stats()
    r = args.reps
    dms, sms = (st.decode_ms - st0.decode_ms) / r, (st.scan_ms - st0.scan_ms) / r
    gbps = buf.numel() / dms / 1e6
    line = "%-7s %9d records, %6.1f MB (%.1f B/record): decode %.3f ms (scan %.3f); wire %.0f GB/s = %.3f of the %.1f TB/s peak" % (
        name, n, buf.numel() / 1e6, buf.numel() / n, dms, sms, gbps, gbps / HBM_PEAK_GBPS, HBM_PEAK_GBPS / 1e3)
    if strings:
        total = int(d.strings(0)[0][-1].item())
        line += "; strings %.1f MB: extract %.3f ms, keydict.encode %.3f ms (%d keys)" % (
            total / 1e6, ext / r * 1e3, enc / r * 1e3, kd.size())
        kd.close()
    print(line, flush=True)
    dec.close()
    return buf.numel()


print("%d records over %d keys, %d timed decodes after one warm-up; whole-decode rates (wire bytes read twice, columns "
      "written once)" % (N, args.keys, args.reps), flush=True)
row = wire.make_schema(["STRING", "LONG", "LONG"], key_field=-1, ts_field=1, cols=[2], fmt="ROWDATA")
var_bytes = N * 65
for name in args.streams.split(","):
    if name == "inline":
        run(name, inline_stream(), N, row, True)
    elif name == "var":
        var_bytes = run(name, var_stream(), N, row, True)
    else:
        buf, n = fixed_stream(var_bytes)
        run(name, buf, n, wire.make_schema(["LONG", "LONG", "LONG"], key_field=0, ts_field=-1, cols=[2]), False)
    torch.cuda.empty_cache()
