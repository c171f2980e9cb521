"""Feature dtype (bf16 feature storage) without a GPU: the launcher's --feature_dtype, the binary's --feature-dtype parsing,
and the new C entry points (declared, exported, in lib.SIGNATURES)."""
import os
import re
import stat
import subprocess

import pytest

from legion_amd import launcher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "legion_hip.h")
LIB = os.path.join(ROOT, "legion_amd", "liblegion_hip.so")
NEW_SYMBOLS = ("legion_feature_create_ex", "legion_feature_dtype", "legion_feature_row_bytes", "legion_feature_table",
               "legion_convert_f32_to_bf16", "legion_server_set_feature_dtype")


def _run_launcher(tmp_path, monkeypatch, extra):
    """Runs launcher.Run against a stand-in binary that records its argv; returns (argv, meta_config text)."""
    fake = tmp_path / "fake_server"
    record = tmp_path / "argv.txt"
    fake.write_text('#!/bin/sh\nfor a in "$0" "$@"; do echo "$a"; done > %s\nexit 0\n' % record)
    fake.chmod(fake.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setattr(launcher, "server_binary", lambda: str(fake))
    monkeypatch.chdir(tmp_path)
    args = launcher.build_argparser().parse_args(["--dataset_name", "products", "--usenvlink", "0"] + extra)
    assert launcher.Run(args) == 0
    return record.read_text().split("\n")[:-1], (tmp_path / "meta_config").read_text(), str(fake)


def test_default_launch_is_unchanged(tmp_path, monkeypatch):
    argv, meta, fake = _run_launcher(tmp_path, monkeypatch, [])
    assert argv == [fake, "2", "0", "25", "10"]
    assert meta == launcher.meta_config_line("./dataset", "products", 8000, 38000000, 2)
    assert launcher.build_argparser().parse_args([]).feature_dtype == "float32"


def test_explicit_float32_is_the_default(tmp_path, monkeypatch):
    argv, _, fake = _run_launcher(tmp_path, monkeypatch, ["--feature_dtype", "float32"])
    assert argv == [fake, "2", "0", "25", "10"]


def test_bfloat16_adds_the_binary_flag(tmp_path, monkeypatch):
    argv, meta, fake = _run_launcher(tmp_path, monkeypatch, ["--feature_dtype", "bfloat16", "--fanout", "15,10,5"])
    assert argv == [fake, "2", "0", "15", "10", "5", "--feature-dtype", "bf16"]
    assert meta == launcher.meta_config_line("./dataset", "products", 8000, 38000000, 2)


@pytest.mark.parametrize("bad", ["bf16", "float16", "fp8", ""])
def test_bad_feature_dtype_is_rejected(bad):
    with pytest.raises(SystemExit):
        launcher.build_argparser().parse_args(["--feature_dtype", bad])


def test_new_symbols_declared_exported_and_typed():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    from legion_amd import lib
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared in legion_hip.h"
        assert name in exported, f"{name} not exported"
        assert name in lib.SIGNATURES, f"{name} not in lib.SIGNATURES"
    assert "#define LEGION_FEATURE_F32 0" in text and "#define LEGION_FEATURE_BF16 1" in text


def test_dtype_setter_accepts_known_values_only():
    from legion_amd import lib
    L = lib.load()
    assert L.legion_server_set_feature_dtype(2) == -1
    assert L.legion_server_set_feature_dtype(-1) == -1
    assert L.legion_server_set_feature_dtype(1) == 0
    assert L.legion_server_set_feature_dtype(0) == 0     # back to the default for this process


def test_engine_rejects_unknown_dtype():
    from legion_amd import engine
    with pytest.raises(ValueError):
        engine.FeatureStorage(1, None, 10, 4, feature_dtype="float16")
    assert [engine.bf16_pitch(d) for d in (1, 7, 8, 100, 128, 602)] == [8, 8, 8, 104, 128, 608]


def test_server_binary_rejects_a_bad_dtype_before_touching_a_device():
    binary = os.path.join(ROOT, "legion_amd", "bin", "sampling_server")
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "legion_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run([binary, "1", "0", "--feature-dtype", "fp16"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=env, timeout=60)
    assert p.returncode == 2, p.stdout
    assert b"--feature-dtype: expected f32 or bf16" in p.stdout
