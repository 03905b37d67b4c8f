"""The C-ABI of DBdust's mask exists in the built library, and the command beside it."""
import ctypes
import os

from conftest import ROOT

SYMBOLS = ("damar_dust_reads", "damar_dust_last", "damar_dust_steps", "damar_dust_release", "damar_dust_limits",
           "damar_host_dust_read", "damar_host_dust_piece", "damar_host_dust_join", "damar_dust_track")


def test_dust_symbols_and_command(built):
    L = ctypes.CDLL(os.path.join(ROOT, "damar_amd", "libdamar_hip.so"))
    for s in SYMBOLS:
        assert hasattr(L, s), s
    assert os.access(os.path.join(ROOT, "damar_amd", "bin", "DBdust"), os.X_OK)


def test_dust_limits(built):
    from damar_amd import api
    piece, halo, stripe, window = api.dust_limits()
    assert window == 64 and halo == 2 * window and piece >= 2 * window and stripe == piece
