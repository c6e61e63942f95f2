"""How large a context's scratch buffers are (fast-dnn_amd/csrc/fdnn_ctx_layout.hpp), checked on the host alone: the
stand-alone checker tests/host/ctx_layout_check.cpp reproduces the recorded table of every count make_ctx computed before the
sizes moved into the header (tests/host/ctx_layout_table.txt), and holds, for every launch the selection (fdnn_select.hpp) can
choose over the suite's net shapes, that what the kernel indexes in each buffer fits the layout.  It is built with the address
and undefined-behaviour sanitizers and run as a child process; planted faults in the layout show that the check has teeth.
CPU only."""
import os
import subprocess

import pytest

from conftest import ROOT

TABLE = os.path.join(ROOT, "tests", "host", "ctx_layout_table.txt")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ctx_layout") / "ctx_layout_check")
    src = os.path.join(ROOT, "tests", "host", "ctx_layout_check.cpp")
    inc = os.path.join(ROOT, "fast-dnn_amd", "csrc")
    cc = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", inc, src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    return exe


def test_context_layout_under_sanitizers(checker):
    run = subprocess.run([checker, TABLE], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ctx layout ok" in run.stdout


# the planted fault and the buffer whose shortfall the check must name
@pytest.mark.parametrize("seed,buffer", [(1, "l.act"), (2, "l.fuse_cnt"), (4, "l.xt_ld"), (5, "l.chain_done")],
                         ids=["no_tile_slack", "half_fuse_counters", "xt_ld_64", "chain_done_from_cap"])
def test_planted_layout_fault_is_caught(checker, seed, buffer):
    run = subprocess.run([checker, TABLE, "--seed", str(seed)], capture_output=True, text=True)
    assert run.returncode == 1, run.stdout + run.stderr
    assert "exceeds " + buffer in run.stderr, run.stderr
    assert "ERROR: " not in run.stderr  # (a shortfall the check reported, not a sanitizer's finding)


def test_chain_counter_slack_tiles_are_not_load_bearing(checker):
    """Planted fault 3 removes only the "+ 2" tiles of the chained launch's counter array.  No launch reaches them (the
    argument is in ctx_layout_check.cpp), so the check passes: the sizing keeps them as slack, it does not rely on them."""
    run = subprocess.run([checker, TABLE, "--seed", "3"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr


SCRATCH_NAMES = ("scr_count", "fuse_cnt", "fuse_flag", "chain_ctl", "chain_done")


def test_every_counter_field_has_a_row_in_the_scratch_table(checker):
    """The scratch audit's table (kCtxScratch, fdnn_ctx_layout.hpp): the checker holds that every counter field of CtxLayout is
    either a row of it or an exemption with its reason (it runs with every invocation above as well); the names it prints
    are the five self-rewinding buffers, and the built library reports the same table (no device needed)."""
    from fast_dnn_amd import api

    run = subprocess.run([checker, "--names"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert tuple(run.stdout.split()) == SCRATCH_NAMES
    assert api.scratch_names() == SCRATCH_NAMES
