"""TKhomogenize on the GPU (kernels/homogenize.hip): every fixture of tests/golden/homogenize/ through the command and the
Python call, equal to the reference's tracks bit for bit; the planted shapes of tests/hom_shapes.py against the model
(tests/hom_model.py) with the counts damar_homog_last reports; the same piles in one batch and in several."""
import pytest

import hom_checks
import hom_common as hc

pytestmark = pytest.mark.gpu
CASES = hc.load_cases("cases") + hc.load_cases("synth")
IDS = [c["name"] for c in CASES]


@pytest.fixture(autouse=True)
def device_path(monkeypatch, built):
    monkeypatch.delenv("DAMAR_PILES", raising=False)
    monkeypatch.delenv("DAMAR_PILE_BATCH", raising=False)
    monkeypatch.delenv("DAMAR_PILE_TRACE_BYTES", raising=False)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_command_on_device(case, tmp_path):
    hc.run_case(case, str(tmp_path), {}, timeout_s=120)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_homogenize_track_on_device(case, tmp_path):
    from damar_amd import api
    hom_checks.check_python_equals_command(case, str(tmp_path), {})
    ms, records, ranges, intervals = api.homog_last()
    assert records > 0 and intervals == len(hc.expected(case["name"])["data"]) // 2 and ms["readout"] > 0


@pytest.mark.parametrize("name", ["def_tiny2", "def_tiny_s", "e2000_tandem", "c12_fusion"])
def test_many_batches_on_device(name, tmp_path, monkeypatch):
    case = [c for c in CASES if c["name"] == name][0]
    monkeypatch.setenv("DAMAR_PILE_BATCH", "500")
    hom_checks.check_python_equals_command(case, str(tmp_path), {})


@pytest.mark.parametrize("name", sorted(hom_checks.SYNTH_KW))
def test_planted_shapes_on_device(name):
    ms = hom_checks.check_synth(name)
    print(name, ms)
    assert ms["mark"] > 0


def test_planted_records_on_device():
    hom_checks.check_roles()


@pytest.mark.parametrize("name", ["synth", "synth_m_r7", "synth_e"])
def test_piles_in_different_batches_on_device(name):
    hom_checks.check_batches(name)


def test_four_piles_in_three_batches_on_device(tmp_path, monkeypatch):
    hom_checks.check_reader_batches(str(tmp_path), monkeypatch)


def test_two_byte_traces_on_device():
    hom_checks.check_two_byte()


def test_empty_batch_list_on_device():
    hom_checks.check_empty_list()
