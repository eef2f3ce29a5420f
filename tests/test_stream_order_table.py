"""The table of the stream-order tests held to the header, on the host: every function of include/ratelib_amd.h whose parameter
list has `hip_stream`, and the handle's *_device calls with RRX_reset and RRX_set_stream, has a row in tests/stream_order_cases.py
(which tests/test_gpu_stream_order.py runs behind gates on the device) or an entry in EXEMPT with a written reason.  A new entry
point without a row fails here."""
import os

import stream_order_cases as SOC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "ratelib_amd.h")) as f:
        return f.read()


def test_the_header_is_parsed():
    free, handle = SOC.header_entries(header())
    # what the parser must find at the least: the first and the last handle-free call of the header, a call whose prototype runs
    # over five lines, and the eleven handle calls
    assert {"RRX_lpc_extrapolate_device", "RRX_tracks_stage_mix_window_device", "RRX_tracks_limit_release_window_device"} <= set(free)
    assert len(free) >= 31 and all(n.endswith("_device") or n.endswith("_device_samples") for n in free), free
    assert len(handle) == 11 and {"RRX_reset", "RRX_set_stream", "RRX_flow_device_samples", "RRX_push_device_double"} <= set(handle), handle
    assert "RRX_device" not in handle and "RRX_sync" not in handle


def test_every_stream_taking_entry_point_has_a_row_or_a_reason():
    free, handle = SOC.header_entries(header())
    rows = SOC.rows()
    missing = [n for n in free if n not in rows and n not in SOC.EXEMPT]
    assert not missing, "entry points that take hip_stream without a row in tests/stream_order_cases.py: %s" % missing
    missing = [n for n in handle if n not in SOC.HANDLE_CALLS and n not in SOC.EXEMPT]
    assert not missing, "handle calls without a row in tests/stream_order_cases.py: %s" % missing
    for n, why in SOC.EXEMPT.items():
        assert isinstance(why, str) and len(why.split()) >= 5, (n, "an exemption needs a written reason")
        assert n not in rows and n not in SOC.HANDLE_CALLS, (n, "is both exempt and in the table")


def test_the_table_names_nothing_the_header_lacks():
    free, handle = SOC.header_entries(header())
    assert not set(SOC.rows()) - set(free) and not set(SOC.HANDLE_CALLS) - set(handle) and not set(SOC.EXEMPT) - set(free) - set(handle)
    # every row says where its seam case is: its own, the one case it has, or none for a launcher without a slice loop
    assert not (set(SOC.SEAM_IS_THE_CASE) | set(SOC.SEAMLESS)) - set(SOC.rows()) and not set(SOC.SEAM_IS_THE_CASE) & set(SOC.SEAMLESS)


def test_a_new_entry_point_would_be_noticed():
    text = header() + "\nint RRX_new_thing_device(int device, void *hip_stream,\n                         const void *d_src, size_t frames);\n"
    free, _ = SOC.header_entries(text)
    assert "RRX_new_thing_device" in free and "RRX_new_thing_device" not in SOC.rows()


def test_every_wrapper_that_takes_a_stream_is_called_behind_gates():
    """every public function of ratelib.py with a `stream` parameter is the wrapper of a row, and every row's wrapper is called
    behind the gates -- by the row itself or by a wrapper row -- or is exempt with a written reason"""
    import inspect

    import foo_dsp_resampler_amd as F
    takes = sorted(n for n, f in vars(F.ratelib).items()
                   if inspect.isfunction(f) and not n.startswith("_") and "stream" in inspect.signature(f).parameters)
    assert takes == sorted(set(SOC.WRAPPER_OF.values())), (takes, sorted(set(SOC.WRAPPER_OF.values())))
    assert set(SOC.WRAPPER_OF) == set(SOC.rows())
    for entry in SOC.rows():
        where = [entry in SOC.WRAPPER_IN_ROW, entry in SOC.WRAPPER_ROWS, entry in SOC.WRAPPER_EXEMPT]
        assert sum(where) == 1, (entry, where)
    for n, why in SOC.WRAPPER_EXEMPT.items():
        assert isinstance(why, str) and len(why.split()) >= 5, (n, "an exemption needs a written reason")


def test_any_return_type_is_parsed():
    text = header() + "\nconst char *RRX_named_device(int device, void *hip_stream);\nunsigned long long RRX_count_device(void *hip_stream,\n    int a);\n"
    free, _ = SOC.header_entries(text)
    assert {"RRX_named_device", "RRX_count_device"} <= set(free)
