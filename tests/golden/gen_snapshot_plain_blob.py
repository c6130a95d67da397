"""Writes tests/golden/snapshot_table_tumble_count_sum.bin: the fwa_snapshot blob of a Table TUMBLE COUNT + SUM_I64
handle, as the build BEFORE the COUNT(DISTINCT) aggregate wrote it.

The committed file was written on an MI355X by commit ef1fe48 ("Tumbling fire: one pass per watermark that also retires
its slices", the parent of the commit that added FWA_COUNT_DISTINCT):

    git checkout ef1fe48 && make -C flink_amd/csrc ARCH=gfx950
    python gen_snapshot_plain_blob.py          # this file, copied into that checkout's tests/golden/

It needs nothing but flink_amd, so it runs unchanged on that commit. tests/test_distinct_snapshot_gpu.py builds the same
blob with the current build and compares the bytes: handles without the aggregate must keep their snapshot format (the
two header words the distinct section uses stay 0 for them). Run on a later build, this script only reproduces what
that test computes; regenerate the file only from ef1fe48.

The handle holds one window and one key per key group, so the order of the entries inside the blob does not depend on
the order in which the GPU emitted them.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "snapshot_table_tumble_count_sum.bin")


def plain_blob(eng_mod):
    from flink_amd import _abi as A
    cand = np.arange(400, dtype=np.int64)
    kgs, _ = eng_mod.key_groups(cand, 128, 1, A.KEY_JAVA_LONG)
    _, first = np.unique(kgs, return_index=True)
    keys = np.repeat(cand[np.sort(first)][:24], 3)
    ts = (np.arange(len(keys), dtype=np.int64) * 37) % 1000
    vals = np.arange(len(keys), dtype=np.int64) * 1_000_003 - 7
    g = eng_mod.WindowAggregator(A.make_config(window_kind="TUMBLE", semantics="TABLE", size_ms=1000,
                                               aggs=[("COUNT", 0), ("SUM_I64", 0)], key_capacity=1024))
    g.push(keys, ts, [vals])
    blob = g.snapshot()
    g.close()
    return blob


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from flink_amd import engine
    with open(OUT, "wb") as f:
        f.write(plain_blob(engine))
