"""The server <-> trainer wire format has one definition, legion_amd/csrc/ipc_wire.h, which the server, the trainer extension and the
protocol-only consumer include.  tests/cpu/ipc_wire_test.cpp pins it over a literal table: the offset of every field of the slab and of
the mirror object, the magic, the version and its thresholds, the slots, the counter indices and every name -- numbers taken from the
structs as they were before the header existed, so a trainer end built then reads a server built now.  tests/cpu/ipc_wire_fds_test.cpp
passes file descriptors through the header's primitives under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own.
Host only: no GPU, no HIP, nothing preloaded."""
import os
import re
import subprocess

from tests import test_sanitizers_cpu as server_end
from tests.rule_table import ROOT, assert_catches, assert_passes, run_table

RESERVED = "    int32_t ext_reserved2;\n"


def test_the_layout_the_numbers_and_the_names_over_a_table(tmp_path):
    assert_passes(run_table(tmp_path, "ipc_wire"))


def test_the_table_catches_a_dropped_field(tmp_path):
    """Without ext_reserved2 the dtype field moves up four bytes (the object keeps its size: 8-byte alignment): the table says so, so the
    test above is able to fail."""
    res = run_table(tmp_path, "ipc_wire", ("ipc_wire.h", RESERVED, ""))
    assert_catches(res)
    assert "MISMATCH feature_out_dtype: got 3508, want 3512" in res.stdout, res.stdout


def test_the_server_end_played_in_python_has_the_pinned_sizes():
    """tests/test_sanitizers_cpu.py creates the slab and the mirror object for the consumer, which maps both at their full size."""
    table = open(os.path.join(ROOT, "tests", "cpu", "ipc_wire_test.cpp")).read()
    pinned = {what: int(want) for what, want in re.findall(r'\{"([^"]+)", (?:sizeof|offsetof)\([^}]*\), (\d+)\}', table)}
    assert (pinned["sizeof(shmStruct)"], pinned["counters"], pinned["sizeof(shmExt)"]) == (7180, 16, 3544)
    assert server_end.SHM_BYTES == pinned["sizeof(shmStruct)"]
    assert server_end.EXT_COUNTERS == pinned["counters"]
    assert server_end.EXT_BYTES == pinned["sizeof(shmExt)"]


def test_descriptor_passing_under_asan_ubsan():
    """1, 64, 65 and 130 descriptors in messages of at most 64, in order, each closed as it arrives; a peer that closes early gives -1."""
    exe = os.path.join(ROOT, "oracle", "_build", "san", "ipc_wire_fds_test")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), exe])
    res = subprocess.run([exe], env=server_end.ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0 and "5 rounds, 0 failed" in res.stdout and "runtime error" not in res.stdout, res.stdout[-3000:]
