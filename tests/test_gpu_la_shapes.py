"""The Local_Alignment kernels, one alignment at a time, at the shapes of tests/la_shapes.py: every task's 12 path integers
and both traces from damar_local_alignment_batch_opts must be IDENTICAL to oracle_local_alignment (integer work: no
tolerance), which tests/test_la_host.py pins to the reference's Local_Alignment on the very same tasks.

Kernel variants (their switches are read once per process, so each runs in ONE fresh child that does all families):

  default     the two-pair kernel (kernels/report_packed.h report2_kernel), the wide kernel behind it where a read has more
              than DAMAR_MAX_MARKS trace spacings
  one_pair    DAMAR_PACKED=0: kernels/report.hip, one task per wavefront.  No wide kernel runs behind that path: reads beyond
              DAMAR_MAX_MARKS spacings are a loud error there (shim.hip marks_must_fit), so the groups `spacing_marks_*` are
              not given to it -- every other group is
  wide        DAMAR_TEST_MAX_CELLS=128: the pebble pool so small that the tasks of more than 128 pebbles a direction overflow
              into the wide kernel (la_batch_kernel<1>); the child's stderr must say `wide kernel`
  t8_limit    DAMAR_TEST_T8_LIMIT=3: byte traces whose values "do not fit", so that the 16-bit repeat happens

`default` and `wide` also run the families of la_shapes.T8_FAMILIES with byte traces (t8 = 1; the groups of tspace <= 125),
the production default that damar_local_alignment_batch cannot reach.

`mixed` runs under DAMAR_SLOTS=16 (2 * 16 + 1 tasks are then "an odd count near twice the slot count"): in the `wide` child
that is a wide launch behind a scratch of fewer slots than the wide pebbles were first sized for (shim.hip wide_slots).

What a family reaches (band widths beyond a half and beyond a wavefront, long passes, whole-read paths, the over-marks task)
is asserted on the ORACLE's statistics by la_shapes.check_reach(), never on the code under test."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import la_shapes as S  # noqa: E402

pytestmark = pytest.mark.gpu

VARIANTS = {
    "default":  {},
    "one_pair": {"DAMAR_PACKED": "0"},
    "wide":     {"DAMAR_TEST_MAX_CELLS": "128"},
    "t8_limit": {"DAMAR_TEST_T8_LIMIT": "3"},
}
T8_LIMIT_FAMILY = "noisy"
FIELDS = ["A abpos", "A bbpos", "A aepos", "A bepos", "A diffs", "A tlen",
          "B abpos", "B bbpos", "B aepos", "B bepos", "B diffs", "B tlen"]


def _runs(variant):
    """(family, t8) the variant's child does"""
    if variant == "t8_limit":
        return [(T8_LIMIT_FAMILY, 1)]
    runs = [(name, 0) for name in S.FAMILIES]
    if variant in ("default", "wide"):
        runs += [(name, 1) for name in S.T8_FAMILIES]
    return runs


def _groups(variant, name, t8):
    out = []
    for gi, g in enumerate(S.family(name)):
        if t8 and g.tspace > 125:
            continue
        if variant == "one_pair" and g.name.startswith("spacing_marks"):
            continue
        out.append((gi, g))
    return out


def _run_group(L, g, t8):
    """-> (per task (12 path integers, A trace, B trace), t8 fell back, tasks answered by the wide kernel)"""
    from damar_amd import api
    adb, bdb = S.make_db(g.areads), S.make_db(g.breads)
    spec = L.New_Align_Spec(g.e, g.tspace, adb.freq, 1, 1, 0, 0, 1)
    ablk, bblk = L.damar_block_upload(C.byref(adb)), L.damar_block_upload(C.byref(bdb))
    nt = len(g.tasks)
    flat = [v for t in g.tasks for v in t]
    paths = (C.c_int * (12 * nt))()
    toff = (api.c_int64 * (2 * nt))()
    cap = nt * 2 * g.maxtp() + 64
    traces = (C.c_uint16 * cap)()
    fell, wide = C.c_int(-1), C.c_int(-1)
    rc = L.damar_local_alignment_batch_opts(ablk, bblk, g.comp, spec, (C.c_int * len(flat))(*flat), nt, paths, toff, traces, cap,
                                            t8, C.byref(fell), C.byref(wide))
    assert rc == 0, (g.name, rc)
    res = []
    for t in range(nt):
        p = list(paths[12 * t:12 * t + 12])
        res.append((p, list(traces[toff[2 * t]:toff[2 * t] + p[5]]), list(traces[toff[2 * t + 1]:toff[2 * t + 1] + p[11]])))
    L.damar_block_free(ablk)
    L.damar_block_free(bblk)
    L.Free_Align_Spec(spec)
    return res, fell.value, wide.value


def _child(variant, out):
    from damar_amd import api
    L = api.lib()
    assert L.damar_hip_init(0) >= 1
    L.Set_Filter_Params(14, 6, 0, 35, 4)
    got = {}
    for name, t8 in _runs(variant):
        if name == "mixed":                                # few slots, so that 2 * slots + 1 tasks are a test-sized batch
            os.environ["DAMAR_SLOTS"] = str(S.MIXED_SLOTS)
        for gi, g in _groups(variant, name, t8):
            got[(name, t8, gi)] = _run_group(L, g, t8)
        os.environ.pop("DAMAR_SLOTS", None)
    with open(out, "wb") as f:
        pickle.dump(got, f)


@pytest.fixture(scope="module")
def gpu(built):
    from damar_amd import api
    L = api.lib()
    assert L.damar_hip_init(0) >= 1
    return L


@pytest.fixture(scope="module")
def reach(built):
    S.check_reach()
    return True


_children = {}


@pytest.fixture(scope="module")
def child(gpu, tmp_path_factory):
    """variant -> (results of its child process, the child's stderr); a child runs once, when first asked for"""
    tmp = tmp_path_factory.mktemp("la_shapes")

    def get(variant):
        if variant not in _children:
            out = str(tmp / (variant + ".pkl"))
            env = {k: v for k, v in os.environ.items() if k not in ("DAMAR_PACKED", "DAMAR_TEST_MAX_CELLS", "DAMAR_TEST_T8_LIMIT", "DAMAR_SLOTS")}
            env.update(VARIANTS[variant])
            r = subprocess.run([sys.executable, os.path.abspath(__file__), variant, out], cwd=ROOT, env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert r.returncode == 0, "child %s: exit %d\n%s\n%s" % (variant, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
            with open(out, "rb") as f:
                _children[variant] = (pickle.load(f), r.stderr)
        return _children[variant]
    return get


def _compare(variant, name, t8, got):
    """every task of every group the variant ran, against the oracle; -> descriptions of the tasks that differ"""
    want = S.oracle(name)
    bad, seen = [], 0
    for gi, g in _groups(variant, name, t8):
        res, _, _ = got[(name, t8, gi)]
        ans = want[gi][0]
        assert len(res) == len(ans) == len(g.tasks)
        for t in range(len(g.tasks)):
            seen += 1
            (gp, gat, gbt), (wp, wat, wbt) = res[t], ans[t]
            what = None
            for i in range(12):
                if gp[i] != wp[i]:
                    what = "%s: got %d, oracle %d" % (FIELDS[i], gp[i], wp[i])
                    break
            if what is None:
                for nm, a, b in (("A trace", gat, list(wat)), ("B trace", gbt, list(wbt))):
                    if a != b:
                        i = next(i for i in range(len(b)) if a[i] != b[i])
                        what = "%s[%d]: got %d, oracle %d" % (nm, i, a[i], b[i])
                        break
            if what is not None:
                bad.append("%s/%s t8=%d %s task %d (%s) reads %s seed %s: %s"
                           % (variant, name, t8, g.name, t, g.tags[t], g.lens(t), g.point(t), what))
    assert seen > 0
    for b in bad[:20]:
        print(b)
    return bad


@pytest.mark.parametrize("name", list(S.FAMILIES))
@pytest.mark.parametrize("variant", ["default", "one_pair", "wide"])
def test_gpu_la_family_equals_oracle(child, reach, variant, name):
    got, err = child(variant)
    bad = _compare(variant, name, 0, got)
    assert not bad, "%d task(s) differ, the first: %s" % (len(bad), bad[0])
    if variant == "wide":
        assert "wide kernel" in err


@pytest.mark.parametrize("name", list(S.T8_FAMILIES))
@pytest.mark.parametrize("variant", ["default", "wide"])
def test_gpu_la_family_with_byte_traces_equals_oracle(child, reach, variant, name):
    """ReportArgs.t8: the device writes the trace values as bytes, the entry widens them; no value of these families is above
    255, so no group may have fallen back to 16 bits"""
    got, err = child(variant)
    bad = _compare(variant, name, 1, got)
    assert not bad, "%d task(s) differ, the first: %s" % (len(bad), bad[0])
    groups = _groups(variant, name, 1)
    assert groups and all(g.tspace <= 125 for _, g in groups)
    assert [got[(name, 1, gi)][1] for gi, _ in groups] == [0] * len(groups)


def test_gpu_la_byte_traces_repeat_at_16_bits_when_a_value_does_not_fit(child, reach):
    """DAMAR_TEST_T8_LIMIT=3 makes every group of the family hold a value "too large for a byte" (any alignment with more
    than 3 differences in a trace segment): DAMAR_ERR_T8, the launch again with 16-bit values, the flag set, the answers
    still the oracle's"""
    got, _ = child("t8_limit")
    bad = _compare("t8_limit", T8_LIMIT_FAMILY, 1, got)
    assert not bad, "%d task(s) differ, the first: %s" % (len(bad), bad[0])
    groups = _groups("t8_limit", T8_LIMIT_FAMILY, 1)
    for gi, g in groups:
        over = any(max(list(at) + list(bt) + [0]) > 3 for _, at, bt in S.oracle(T8_LIMIT_FAMILY)[gi][0])
        assert over and got[(T8_LIMIT_FAMILY, 1, gi)][1] == 1, g.name


@pytest.mark.parametrize("variant,t8", [("default", 0), ("default", 1), ("wide", 0), ("wide", 1)])
def test_gpu_la_reads_beyond_the_packed_marks_go_to_the_wide_kernel(child, reach, variant, t8):
    """the 20 kb pair at a spacing of one base has more than DAMAR_MAX_MARKS trace spacings: its task is the wide kernel's by
    read length (the entry returns DAMAR_CNT_WIDE); the groups of ordinary reads at the default pool size leave it nothing"""
    got, _ = child(variant)
    marks = [(gi, g) for gi, g in _groups(variant, "spacing", t8) if g.name.startswith("spacing_marks")]
    assert len(marks) == 2
    for gi, g in marks:
        assert got[("spacing", t8, gi)][2] == len(g.tasks) == 1
    if variant == "default":
        for name in ("noisy", "ends") + (() if t8 else ("short",)):
            assert [got[(name, t8, gi)][2] for gi, _ in _groups(variant, name, t8)] == [0] * len(_groups(variant, name, t8))


if __name__ == "__main__":                                 # the child: every family on the path the environment selects
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    _child(sys.argv[1], sys.argv[2])
