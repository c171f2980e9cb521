"""The runner of the host-only rule tables: tests/cpu/<name>_test.cpp pins one header of legion_amd/csrc over a literal table, prints
MISMATCH per wrong entry and "N failed" at the end.  run_table compiles and runs one, optionally against a COPY of one header with a rule
replaced -- which is how each table proves that it is able to fail.  Host only: no torch, no HIP."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "legion_amd", "csrc")
INCLUDE = re.compile(r'#include "([^"]+)"')


def _absolute(text):
    """text with every #include "X" that names an existing file, seen from legion_amd/csrc, naming it by its absolute path: a copy in
    another directory then finds what the original found."""
    def one(m):
        path = os.path.normpath(os.path.join(CSRC, m.group(1)))
        return '#include "%s"' % path if os.path.isfile(path) else m.group(0)
    return INCLUDE.sub(one, text)


def run_table(tmp_path, name, mutate=None):
    """Compile and run tests/cpu/<name>_test.cpp; the CompletedProcess.  mutate = (header, old, new[, times]): the table is compiled
    against a copy of legion_amd/csrc/<header> in which `old`, found exactly `times` times (once), is `new`."""
    src = os.path.join(ROOT, "tests", "cpu", name + "_test.cpp")
    if mutate is not None:
        header, old, new, times = (tuple(mutate) + (1,))[:4]
        text = open(os.path.join(CSRC, header)).read()
        assert text.count(old) == times, (header, old, text.count(old))
        copy = tmp_path / header
        copy.write_text(_absolute(text.replace(old, new)))
        test = open(src).read()
        theirs = '#include "../../legion_amd/csrc/%s"' % header
        assert test.count(theirs) == 1, (name, header)
        # tests/cpu lies two directories below the root, as legion_amd/csrc does: the test's other includes resolve alike
        test = _absolute(test.replace(theirs, '#include "%s"' % copy))
        src = str(tmp_path / "t.cpp")
        open(src, "w").write(test)
    exe = str(tmp_path / (name + "_test"))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe], cwd=tmp_path)
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


def assert_passes(res):
    assert res.returncode == 0 and " 0 failed" in res.stdout, res.stdout[-3000:]


def assert_catches(res):
    assert res.returncode != 0 and "MISMATCH" in res.stdout, res.stdout[-3000:]
