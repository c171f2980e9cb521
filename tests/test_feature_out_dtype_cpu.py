"""Feature output dtype (bf16 rows handed to the trainer) without a GPU: the launcher's --trainer_feature_dtype, the binary's
--feature-out-dtype parsing, the new C entry points (declared, exported, in lib.SIGNATURES) and the refusals the C ABI makes
before any device is touched."""
import os
import re
import stat
import subprocess

import pytest

from legion_amd import launcher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "legion_hip.h")
LIB = os.path.join(ROOT, "legion_amd", "liblegion_hip.so")
NEW_SYMBOLS = ("legion_pool_set_feature_out_dtype", "legion_pool_feature_out_dtype", "legion_pipeline_create_ex",
               "legion_server_set_feature_out_dtype")


def _run_launcher(tmp_path, monkeypatch, extra):
    """Runs launcher.Run against a stand-in binary that records its argv; returns (argv, meta_config text, binary)."""
    fake = tmp_path / "fake_server"
    record = tmp_path / "argv.txt"
    fake.write_text('#!/bin/sh\nfor a in "$0" "$@"; do echo "$a"; done > %s\nexit 0\n' % record)
    fake.chmod(fake.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setattr(launcher, "server_binary", lambda: str(fake))
    monkeypatch.chdir(tmp_path)
    args = launcher.build_argparser().parse_args(["--dataset_name", "products", "--usenvlink", "0"] + extra)
    assert launcher.Run(args) == 0
    return record.read_text().split("\n")[:-1], (tmp_path / "meta_config").read_text(), str(fake)


def test_default_trainer_dtype_leaves_the_launch_unchanged(tmp_path, monkeypatch):
    argv, meta, fake = _run_launcher(tmp_path, monkeypatch, ["--trainer_feature_dtype", "float32"])
    assert argv == [fake, "2", "0", "25", "10"]
    assert meta == launcher.meta_config_line("./dataset", "products", 8000, 38000000, 2)
    assert launcher.build_argparser().parse_args([]).trainer_feature_dtype == "float32"


@pytest.mark.parametrize("storage,flags", [("float32", []), ("bfloat16", ["--feature-dtype", "bf16"])])
def test_bfloat16_trainer_rows_add_the_binary_flag(tmp_path, monkeypatch, storage, flags):
    argv, meta, fake = _run_launcher(tmp_path, monkeypatch, ["--feature_dtype", storage, "--trainer_feature_dtype", "bfloat16",
                                                             "--fanout", "15,10,5"])
    assert argv == [fake, "2", "0", "15", "10", "5"] + flags + ["--feature-out-dtype", "bf16"]
    assert meta == launcher.meta_config_line("./dataset", "products", 8000, 38000000, 2)


@pytest.mark.parametrize("bad", ["bf16", "float16", "fp8", ""])
def test_bad_trainer_dtype_is_rejected(bad):
    with pytest.raises(SystemExit):
        launcher.build_argparser().parse_args(["--trainer_feature_dtype", bad])


def test_new_symbols_declared_exported_and_typed():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    from legion_amd import lib
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared in legion_hip.h"
        assert name in exported, f"{name} not exported"
        assert name in lib.SIGNATURES, f"{name} not in lib.SIGNATURES"


def test_setters_accept_known_values_only():
    from legion_amd import lib
    L = lib.load()
    for bad in (2, -1, 7):
        assert L.legion_server_set_feature_out_dtype(bad) == -1
        assert L.legion_pool_set_feature_out_dtype(None, bad) == -1
    assert L.legion_server_set_feature_out_dtype(1) == 0
    assert L.legion_server_set_feature_out_dtype(0) == 0     # back to the default for this process
    assert L.legion_pool_set_feature_out_dtype(None, 1) == -1      # no pool
    assert L.legion_pool_feature_out_dtype(None) == -1


def test_engine_rejects_unknown_out_dtype():
    from legion_amd import engine
    with pytest.raises(ValueError):
        engine.MemoryPool(0, 10, 4, [2], 4, feature_out_dtype="float16")
    with pytest.raises(ValueError):
        engine.Pipeline(None, None, None, 0, 4, [2], 1, 8, feature_out_dtype="bf16")


@pytest.mark.parametrize("value", ["fp16", "", "bfloat16"])
def test_server_binary_rejects_a_bad_out_dtype_before_touching_a_device(value):
    binary = os.path.join(ROOT, "legion_amd", "bin", "sampling_server")
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "legion_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run([binary, "1", "0", "--feature-out-dtype", value], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=env, timeout=60)
    assert p.returncode == 2, p.stdout
    assert b"--feature-out-dtype: expected f32 or bf16" in p.stdout


def test_usage_line_names_the_flag():
    binary = os.path.join(ROOT, "legion_amd", "bin", "sampling_server")
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "legion_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run([binary], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=60)
    assert p.returncode == 2 and b"[--feature-out-dtype f32|bf16]" in p.stdout
