"""The C-ABI of OGbuild's edges exists in the built library, and the command beside it."""
import ctypes
import os

from conftest import ROOT

SYMBOLS = ("damar_graph_open", "damar_graph_batch", "damar_graph_finish", "damar_graph_close", "damar_graph_last", "damar_graph_maxdeg",
           "damar_graph_result_free", "damar_host_graph_open", "damar_host_graph_batch", "damar_host_graph_finish", "damar_host_graph_close",
           "damar_host_graph_dedupe", "damar_og_build", "damar_og_edges")


def test_og_symbols_and_command(built):
    L = ctypes.CDLL(os.path.join(ROOT, "damar_amd", "libdamar_hip.so"))
    for s in SYMBOLS:
        assert hasattr(L, s), s
    assert os.access(os.path.join(ROOT, "damar_amd", "bin", "OGbuild"), os.X_OK)
    from damar_amd import api
    assert callable(api.og_build) and callable(api.og_edges) and callable(api.og_last)
