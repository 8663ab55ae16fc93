"""rnnl_paths_rows on the host: the library exports the two calls,
the constants of _native are the header's, bad arguments are refused with
RNNL_ERR_INVALID and a message before a device is touched, the Python checks of
explain_paths and predict(paths=) raise without a device, the line format of the
predictions file with paths, and the in-edge builder of graph.cpp under
AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program.
Needs no GPU.
"""
import ctypes
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

from rnnlogic_amd import _native
from rnnlogic_amd import predictors, trainer

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def last_error():
    return _native.lib().rnnl_last_error().decode()


def test_library_exports_the_calls():
    names = [n for n, _, _ in _native.SIGNATURES]
    for name in ("rnnl_paths_rows", "rnnl_paths_rows_scratch"):
        assert hasattr(_native.lib(), name)
        assert name in names


def test_constants_are_the_headers():
    text = open(os.path.join(REPO, "include", "rnnlogic_hip.h")).read()
    assert int(re.search(r"#define RNNL_PATHS_MAX (\d+)", text).group(1)) == _native.PATHS_MAX == 64
    assert int(re.search(r"#define RNNL_PATH_LEN (\d+)", text).group(1)) == _native.PATH_LEN == 6


def paths_rows(g=None, r=None, arrays=False, n=1, m=3, c=3, P=3, counters=True):
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)
    a = p if arrays else None
    return _native.lib().rnnl_paths_rows(g, r, a, a, None, n, a, m, a, c, P, a, a, a, None, 0,
                                         p if counters else None, None)


@pytest.mark.parametrize("kw,word", [
    (dict(m=0), "m ("), (dict(m=-3), "m ("), (dict(c=0), "c ("), (dict(c=17), "c ("),
    (dict(P=0), "max_paths"), (dict(P=65), "max_paths"), (dict(P=-1), "max_paths"),
    (dict(), "handle"), (dict(arrays=True), "handle")])
def test_bad_arguments_are_refused_before_a_handle_is_read(kw, word):
    """With a null handle (and null arrays) every scalar out of range is named
    in the message: it was decided first, nothing was dereferenced."""
    assert paths_rows(**kw) == _native.RNNL_ERR_INVALID
    assert "rnnl_paths_rows" in last_error() and word in last_error()


def test_scratch_size_needs_a_graph():
    need = ctypes.c_size_t(7)
    assert _native.lib().rnnl_paths_rows_scratch(None, 1, ctypes.byref(need)) == _native.RNNL_ERR_INVALID
    assert "rnnl_paths_rows_scratch" in last_error() and need.value == 7


def fake_model():
    m = object.__new__(predictors.Predictor)  # (no torch.nn.Module state is needed for the argument checks)
    return m


def test_python_checks_need_no_device():
    m = fake_model()
    h, r = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
    ent, rules = torch.zeros((1, 2), dtype=torch.int32), torch.zeros((1, 2, 3), dtype=torch.int32)
    for P in (0, 65, -2):
        with pytest.raises(ValueError, match="max_paths must be 1..64"):
            m.explain_paths(h, r, ent, rules, P)
    # (the inputs are looked at after max_paths: a CPU tensor is refused as by every forward)
    with pytest.raises(RuntimeError, match="HIP path"):
        m.explain_paths(h, r, ent, rules, 3)


def fake_trainer():
    t = object.__new__(trainer.TrainerPredictor)
    t.device = torch.device("cpu")
    graph = types.SimpleNamespace(id2entity={0: "ann", 1: "bob", 2: "cy", 3: "dee", 4: "eve"},
                                  id2relation={0: "likes", 1: "knows"})
    t.model = types.SimpleNamespace(graph=graph, rules=[(0, [1, 0]), (0, [1]), (1, [0])])
    return t


def test_predict_refuses_paths_without_explain():
    t = fake_trainer()
    with pytest.raises(ValueError, match="explain > 0"):
        t.predict("test", k=3, explain=0, paths=2)
    with pytest.raises(ValueError, match="paths must be 0..64"):
        t.predict("test", k=3, explain=2, paths=65)
    with pytest.raises(ValueError, match="paths must be 0..64"):
        t.predict("test", k=3, explain=2, paths=-1)


def hand_made(with_paths):
    out = dict(h=np.asarray([0]), r=np.asarray([0]), t=np.asarray([1]), index=np.asarray([[1, 4]], dtype=np.int32),
               score=np.asarray([[1.5, 0.25]], dtype=np.float32), valid=np.asarray([2], dtype=np.int32),
               position=np.asarray([0], dtype=np.int32), explain_off=np.asarray([0, 2], dtype=np.int64),
               explain_rule=np.asarray([1, 0]), explain_count=np.asarray([1, 3]))
    if with_paths:
        path = np.full((1, 1, 1, 2, 6), -1, dtype=np.int32)
        path[0, 0, 0, 0, :3], path[0, 0, 0, 1, :3] = (0, 2, 1), (0, 3, 1)
        out.update(explain_path=path, explain_paths_rule=np.asarray([[[0]]], dtype=np.int32),
                   explain_paths_listed=np.asarray([[[2]]], dtype=np.int32),
                   explain_paths_count=np.asarray([[[3]]], dtype=np.int64))
    return out


def test_prediction_lines_with_and_without_paths(tmp_path):
    t = fake_trainer()
    t._write_predictions(str(tmp_path / "plain.tsv"), hand_made(False), 1)
    t._write_predictions(str(tmp_path / "paths.tsv"), hand_made(True), 1)
    assert (tmp_path / "plain.tsv").read_text().splitlines() == [
        "ann\tlikes\t1\tbob\t1.5\t*\tlikes <- knows, likes:3", "ann\tlikes\t2\teve\t0.25\t"]
    assert (tmp_path / "paths.tsv").read_text().splitlines() == [
        "ann\tlikes\t1\tbob\t1.5\t*\tlikes <- knows, likes:3 [ann > cy > bob | ann > dee > bob | ...]",
        "ann\tlikes\t2\teve\t0.25\t"]


def test_top_rules_order():
    """The first m rules of each slot of explain_rows' CSR by (count descending,
    rule id ascending): the order of the file's columns."""
    m = fake_model()
    off = torch.tensor([0, 4, 4, 5, 8])
    rule = torch.tensor([2, 5, 7, 9, 3, 1, 4, 6])
    count = torch.tensor([1, 8, 8, 2, 6, 5, 5, 2 ** 40])
    got = m.top_rules(off, rule, count, 3)
    assert got.dtype == torch.int32
    assert got.tolist() == [[5, 7, 9], [-1, -1, -1], [3, -1, -1], [6, 1, 4]]
    assert m.top_rules(torch.zeros(3, dtype=torch.int64), rule[:0], count[:0], 2).tolist() == [[-1, -1], [-1, -1]]


def test_listable_masks_the_rules_explain_paths_cannot_walk():
    m = fake_model()
    m.rules = [(0, [1]), (0, []), (1, [0] * 5), (1, [0] * 6)]
    named = torch.tensor([[[0, 1, -1], [3, 2, 0]]], dtype=torch.int32)
    got = m.listable(named)
    assert got.dtype == torch.int32 and got.tolist() == [[[0, -1, -1], [-1, 2, 0]]]
    m.rules = []
    assert m.listable(torch.full((1, 1, 2), -1, dtype=torch.int32)).tolist() == [[[-1, -1]]]


@pytest.mark.skipif(shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"),
                    reason="needs g++ and the ROCm headers")
def test_in_edge_builder_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "in_edges_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           os.path.join(HERE, "asan", "in_edges_check.cpp"), os.path.join(REPO, "rnnlogic_amd", "csrc", "graph.cpp"),
           "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    # (the program is linked against the sanitizer's runtime itself; the link-order check is off as in
    # test_host_sanitizers.py, for environments that preload a library of their own into every process)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "0 live blocks" in run.stdout
    print(run.stdout.strip())
