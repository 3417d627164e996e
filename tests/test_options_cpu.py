"""The library's tuning options on the host (no GPU): every name the C ABI has accepted so far, written out here
and not read from the library, still reads -1 when unset, round-trips a value, stores -1 for a negative one and
is -1 again afterwards; a name the library does not know, or none, is refused with the message it always had.

The names and their enumerators come from one list in csrc/common.h; a name lost, misspelt or moved against its
enumerator there shows here (a moved one as another option answering: the values below differ per name)."""
import re

import pytest

from bm2f_amd import _native

OPTION_NAMES = [
    "msda_threads", "msda_tile", "msda_tile_w", "msda_halo", "msda_win_rows", "msda_bwd_tiled", "msda_fwd_tiled",
    "mattn_dq_atomic", "gemm_nt_cfg", "x3_tn_nw", "x3_tn_blocks", "x3_nt_cfg", "msda_fwd_quad", "msda_bwd_overlap",
    "msda_bwd_det", "msda_fwd_pb", "msda_bwd_ratio", "msda_fwd_lds", "msda_fwd_tile", "msda_fwd_tile_w",
    "msda_fwd_cap", "msda_fwd_halo", "mattn_fwd_minblk", "mattn_bwd_minblk", "mask_df_stage",
    "mattn_bwd_keys", "mattn_xcd", "mattn_combine", "msda_bwd_rowsort", "msda_bwd_walk4", "msda_fwd_xcd", "msda_fwd_pair",
    "infer_video_cap"]


def test_option_list_is_the_33_names():
    assert len(OPTION_NAMES) == 33 and len(set(OPTION_NAMES)) == 33


@pytest.mark.parametrize("name", OPTION_NAMES)
def test_option_unset_roundtrip_negative_reset(name):
    i = OPTION_NAMES.index(name)
    assert _native.get_option(name) == -1
    try:
        _native.set_option(name, 100 + i)
        assert _native.get_option(name) == 100 + i
        _native.set_option(name, 2 ** 40 + i)  # the value is 64 bits wide
        assert _native.get_option(name) == 2 ** 40 + i
        _native.set_option(name, 0)
        assert _native.get_option(name) == 0
        _native.set_option(name, -7)
        assert _native.get_option(name) == -1
    finally:
        _native.set_option(name, -1)
    assert _native.get_option(name) == -1


def test_options_are_independent():
    """Each name answers for its own slot: all set at once to different values, all read back, all reset."""
    try:
        for i, name in enumerate(OPTION_NAMES):
            _native.set_option(name, 1000 + i)
        assert [_native.get_option(n) for n in OPTION_NAMES] == [1000 + i for i in range(len(OPTION_NAMES))]
    finally:
        for name in OPTION_NAMES:
            _native.set_option(name, -1)
    assert [_native.get_option(n) for n in OPTION_NAMES] == [-1] * len(OPTION_NAMES)


@pytest.mark.parametrize("name, shown", [("no_such_option", "no_such_option"), ("", ""), ("msda_tile ", "msda_tile "),
                                         (None, "(null)")])
def test_unknown_option_is_refused(name, shown):
    arg = None if name is None else name.encode()
    with pytest.raises(_native.NativeError, match=r"m2f_set_option: unknown option '%s'$" % re.escape(shown)):
        _native.call("m2f_set_option", arg, 1)
    with pytest.raises(_native.NativeError, match=r"m2f_get_option: unknown option '%s'$" % re.escape(shown)):
        _native.query("m2f_get_option", arg)
