"""hgp_band_fused_tile without a device: the {SEG, TW} of the built fused banded kernel."""
import ctypes


def test_tile_is_positive_multiples_of_16():
    from hipgp_amd import _lib
    t = (ctypes.c_int * 2)(-1, -1)
    _lib.check(_lib.lib().hgp_band_fused_tile(t))
    assert t[0] > 0 and t[1] > 0 and t[0] % 16 == 0 and t[1] % 16 == 0, (t[0], t[1])


def test_tile_refuses_a_null_pointer():
    from hipgp_amd import _lib
    assert _lib.lib().hgp_band_fused_tile(None) != 0
