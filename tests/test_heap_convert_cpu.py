"""The host conversion of flink_amd/csrc/heap_snapshot.cpp (Flink heap bytes <-> FWASNAP1 words) without a GPU:
tools/heap_convert_check.cpp links it against stub engine / dictionary entry points, is built here with the host
AddressSanitizer and UndefinedBehaviorSanitizer, and is fed the key-group section of the reference's own reduce
checkpoint (String keys, Tuple2<String, Integer>), every truncation and single-byte damage of it, and hand-made session
blobs. Any sanitizer report aborts the program, which fails the test."""
import os
import subprocess

import heap_reader as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_heap_conversion_stand_alone_under_sanitizers(tmp_path):
    f = os.path.join(ROOT, "tests", "golden", "flink_snapshots", "win-op-migration-test-reduce-event-time-flink1.18-snapshot")
    first, offs, data = H.read_operator_snapshot(open(f, "rb").read())[0]
    sec = tmp_path / "section.bin"
    sec.write_bytes(data[offs[0]:])
    exe = str(tmp_path / "heap_convert_check")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "heap_convert_check.cpp"),
                           os.path.join(ROOT, "flink_amd", "csrc", "heap_snapshot.cpp"), "-o", exe])
    r = subprocess.run([exe, str(sec)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-4000:]
