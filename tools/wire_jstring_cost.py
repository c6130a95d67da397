"""What a String-keyed DataStream channel costs on the GPU (FWA_FIELD_JSTRING): decode, extraction of the key's char
bytes, String.hashCode() (fwa_jstring_hash), key dictionary encode, and the encoder writing the keys back, for
Tuple2<String, Long> StreamRecords with timestamps in a device-resident stream.

Streams (built on the device; 2^24 records, keys uniform over --keys distinct values, one watermark element at the end):
  five   every key 5 ASCII chars: 27-byte elements of one size (be32 L | tag | be64 ts | 06 + 5 chars | be64 v), so the
         walk speculates as on fixed rows
  var    keys of 8..40 ASCII chars (length and content functions of the key): 30..62-byte elements whose sizes differ
         from record to record, so the walk lists elements by scalar steps
Numbers per stream, mean of --reps rounds after one warm-up:
  decode_ms / scan_ms   fwa_wire_stats (HIP events on the decoder's stream: scan + compose + resolve + decode; scan alone)
  extract_ms            fwa_wire_strings_of of the key field: device scan of the lengths + gather (host clock around a
                        call that ends in a synchronise)
  hash_ms               jstring_hash of the extracted values (host clock, likewise)
  dict_ms               KeyDictionary.encode of the extracted values (host clock, likewise)
  encode_ms             fwa_wire_enc_stats of writing (String key, Long v) records with timestamps from the extracted
                        values and the decoded column: size + scan + write passes (HIP events on the encoder's stream);
                        the output is byte for byte the input's records
  wire GB/s             wire bytes / decode_ms and / encode_ms: whole-pass rates (the decoder reads the wire bytes twice
                        and writes the columns once; the encoder reads the values twice and writes every byte once), not
                        one kernel's share of the 8.0 TB/s peak.
Output: python tools/wire_jstring_cost.py > profiles/<tag>_wire_jstring_cost.txt"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flink_amd import _abi as A  # noqa: E402
from flink_amd import wire  # noqa: E402
from flink_amd.keydict import KeyDictionary  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--records", type=int, default=1 << 24)
ap.add_argument("--keys", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--streams", default="five,var")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("wire_jstring_cost.py measures on the GPU: none found")
dev = torch.device("cuda", 0)
HBM_PEAK_GBPS = 8000.0
N = args.records
g = torch.Generator(device=dev)
g.manual_seed(0x5eed)
keys = torch.randint(0, args.keys, (N,), device=dev, generator=g, dtype=torch.int64)
ts = 1_700_000_000_000 + torch.arange(N, device=dev, dtype=torch.int64) // 1000
vals = torch.randint(0, 1 << 31, (N,), device=dev, generator=g, dtype=torch.int64)
WM = torch.tensor([0, 0, 0, 9, 2, 0, 0, 1, 0x8B, 0xCF, 0xE5, 0x68, 0], dtype=torch.uint8, device=dev)   # watermark element


def be(x):   # int64 -> its 8 big-endian bytes per element
    return x.contiguous().view(torch.uint8).view(-1, 8).flip(1)


def hexchar(j):   # ASCII of hex digit j % 5 of the key: 5 digits tell 2^20 keys apart
    nib = (keys >> (4 * (j % 5))) & 15
    return torch.where(nib < 10, nib + 48, nib + 87).to(torch.uint8)


def five_stream():
    rec = torch.zeros(N, 27, dtype=torch.uint8, device=dev)
    rec[:, 3] = 23                                               # be32 L | TAG_REC_WITH_TIMESTAMP (0)
    rec[:, 5:13] = be(ts)
    rec[:, 13] = 6                                               # len + 1
    for j in range(5):
        rec[:, 14 + j] = hexchar(j)
    rec[:, 19:27] = be(vals)
    return torch.cat([rec.reshape(-1), WM])


def var_stream():
    ln = 8 + keys % 33
    esz = 22 + ln
    start = torch.cumsum(esz, 0) - esz
    out = torch.zeros(int(esz.sum().item()) + 13, dtype=torch.uint8, device=dev)
    out[start + 3] = (18 + ln).to(torch.uint8)
    out[start + 13] = (ln + 1).to(torch.uint8)
    tb, vb = be(ts), be(vals)
    for j in range(8):
        out[start + 5 + j] = tb[:, j]
        out[start + 14 + ln + j] = vb[:, j]
    for j in range(40):
        m = ln > j
        out[(start + 14 + j)[m]] = hexchar(j)[m]
    out[-13:] = WM
    return out


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def run(name, buf):
    dec = wire.WireDecoder(wire.make_schema(["JSTRING", "LONG"], key_field=-1, cols=[1], max_bytes=buf.numel()))
    enc = wire.WireEncoder(wire.make_out_schema([("JSTRING", ("KEYCOL", 0, "STRING")), ("LONG", ("AGG", 0, "SUM_I64"))],
                                                record_ts="WIN_TIME", max_bytes=buf.numel()))
    kd = KeyDictionary(["STRING"], capacity=2 * args.keys)
    ext = hsh = dic = 0.0
    st0 = es0 = None
    win_end = ts + 1                                             # record timestamp = win_end - 1
    for rep in range(args.reps + 1):
        d = dec.decode(buf)
        assert d.n_records == N and d.n_events == 1 and d.consumed == buf.numel()
        (offs, data, nul), t_ext = timed(lambda: d.strings(0))
        _, t_hash = timed(lambda: wire.jstring_hash(offs, data))
        _, t_dict = timed(lambda: kd.encode([(offs, data)]))
        out = A.Out()
        out.n_rows, out.on_device, out.num_aggs = N, 1, 1
        out.win_end, out.agg[0] = win_end.data_ptr(), d.cols[0].data_ptr()
        back = enc.encode(out, keycols=([(offs, data)], None), events=[(2, (1_700_000_016_777,))])
        if rep == 0:
            assert torch.equal(back[:-13], buf[:-13]), "the encoder's records differ from the input's"
            st0, es0 = dec.stats(), enc.stats()
        else:
            ext, hsh, dic = ext + t_ext, hsh + t_hash, dic + t_dict
    st, es = dec.stats(), enc.stats()
    r = args.reps
    dms, sms = (st.decode_ms - st0.decode_ms) / r, (st.scan_ms - st0.scan_ms) / r
    ems, ezs, ess = (es.encode_ms - es0.encode_ms) / r, (es.size_ms - es0.size_ms) / r, (es.scan_ms - es0.scan_ms) / r
    total = int(offs[-1].item())
    print("%-5s %9d records, %6.1f MB (%.1f B/record): decode %.3f ms (scan %.3f); wire %.0f GB/s = %.3f of the %.1f TB/s "
          "peak; key chars %.1f MB: extract %.3f ms, jstring_hash %.3f ms, keydict.encode %.3f ms (%d keys); encode %.3f ms "
          "(size %.3f, scan %.3f), wire %.0f GB/s" % (
              name, N, buf.numel() / 1e6, buf.numel() / N, dms, sms, buf.numel() / dms / 1e6,
              buf.numel() / dms / 1e6 / HBM_PEAK_GBPS, HBM_PEAK_GBPS / 1e3, total / 1e6, ext / r * 1e3, hsh / r * 1e3,
              dic / r * 1e3, kd.size(), ems, ezs, ess, buf.numel() / ems / 1e6), flush=True)
    for x in (dec, enc, kd):
        x.close()


print("%d records over %d keys, %d timed rounds after one warm-up; whole-pass rates" % (N, args.keys, args.reps), flush=True)
for name in args.streams.split(","):
    run(name, five_stream() if name == "five" else var_stream())
    torch.cuda.empty_cache()
