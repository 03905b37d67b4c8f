"""What damar_align_boxes, damar_align_reads and damar_trace_boxes refuse before any box is aligned, without a GPU: the three
entry points check a batch with one routine of the shim (damar_amd/csrc/stages/boxes.hip, box_batch_valid), and the lines it writes
to stderr are held here word for word.  Every call is on the host route, so nothing reaches a device."""
import ctypes as C

import numpy as np
import pytest

I64P = C.POINTER(C.c_int64)
# entry point -> (the family's word in its messages, the stage of its damar_*_last)
ENTRIES = dict(damar_align_boxes=("boxes", "box"), damar_align_reads=("reads", "read"), damar_trace_boxes=("trace boxes", "tbox"))
NBASES = 10


@pytest.fixture(autouse=True)
def host_path(monkeypatch):
    for k in ("DAMAR_TRIM", "DAMAR_STITCH", "DAMAR_POSTRACE"):
        monkeypatch.setenv(k, "host")


def call(entry, m, n, aoff, boff, abpos=None, nbox=None, out=True):
    """one call of `entry` on boxes inside NBASES bases -> (the return value, the counters of its damar_*_last)"""
    from damar_amd import api
    L = api.lib()
    PI = C.POINTER(C.c_int)
    m, n = (np.asarray(x, dtype=np.int32) for x in (m, n))
    aoff, boff = (np.asarray(x, dtype=np.int64) for x in (aoff, boff))
    ab = np.asarray(abpos if abpos is not None else [0] * len(m), dtype=np.int32)
    bases = np.zeros(NBASES, dtype=np.uint8)
    nb = len(m) if nbox is None else nbox
    diffs, off = np.zeros(len(m) + 1, dtype=np.int32), np.zeros(len(m) + 2, dtype=np.int64)
    if entry == "damar_trace_boxes":
        batch = api.TBoxBatch(nb, m.ctypes.data_as(PI), n.ctypes.data_as(PI), ab.ctypes.data_as(PI), aoff.ctypes.data_as(I64P),
                              boff.ctypes.data_as(I64P), bases.ctypes.data, NBASES, 100)
        res = C.POINTER(C.c_uint16)()
    else:
        batch = api.BoxBatch(nb, m.ctypes.data_as(PI), n.ctypes.data_as(PI), aoff.ctypes.data_as(I64P), boff.ctypes.data_as(I64P),
                             bases.ctypes.data, NBASES)
        res = PI()
    rc = getattr(L, entry)(C.byref(batch), diffs.ctypes.data_as(PI), off.ctypes.data_as(I64P), C.byref(res) if out else None)
    if rc == 0:
        C.CDLL(None).free(res)
    return rc, api._last(ENTRIES[entry][1], 3)[1:]


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_null_output_pointer(entry, capfd):
    assert call(entry, [3], [4], [0], [3], out=False)[0] == 1
    assert capfd.readouterr().err == "damar: %s: malformed batch\n" % ENTRIES[entry][0]


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_negative_box_count(entry, capfd):
    assert call(entry, [3], [4], [0], [3], nbox=-1)[0] == 1
    assert capfd.readouterr().err == "damar: %s: malformed batch\n" % ENTRIES[entry][0]


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_box_without_a_base_of_a(entry, capfd):
    assert call(entry, [3, 0], [4, 2], [0, 7], [3, 7], abpos=[0, 5])[0] == 1
    at = " at 5" if entry == "damar_trace_boxes" else ""
    assert capfd.readouterr().err == "damar: %s: box 1 (0 x 2%s) does not lie inside the 10 bases\n" % (ENTRIES[entry][0], at)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_box_one_base_past_the_end(entry, capfd):
    assert call(entry, [3, 4], [3, 1], [0, 7], [3, 6], abpos=[0, 5])[0] == 1                # 7 + 4 is one past the 10 bases
    at = " at 5" if entry == "damar_trace_boxes" else ""
    assert capfd.readouterr().err == "damar: %s: box 1 (4 x 1%s) does not lie inside the 10 bases\n" % (ENTRIES[entry][0], at)


def test_box_that_begins_in_front_of_a(capfd):
    assert call("damar_trace_boxes", [3], [4], [0], [3], abpos=[-1])[0] == 1
    assert capfd.readouterr().err == "damar: trace boxes: box 0 (3 x 4 at -1) does not lie inside the 10 bases\n"


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_boxes_up_to_the_last_base_are_taken(entry, capfd):
    rc, counters = call(entry, [3, 3], [4, 1], [0, 7], [3, 9], abpos=[0, 5])               # 7 + 3 and 9 + 1 end on the last base
    assert rc == 0 and counters[:2] == (2, 0)
    assert capfd.readouterr().err == ""


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_empty_batch(entry, capfd):
    assert call(entry, [], [], [], []) == (0, (0, 0, 0))
    assert capfd.readouterr().err == ""
