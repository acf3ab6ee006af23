"""The library's runtime options (sn_set_option / sn_get_option, include/scenenet_hip.h) and _hip.options, on the host (no
GPU).  Every case runs in a fresh child process with an environment of its own: an option's variable is read once per
process, at the first look at the option, and nothing set here leaks into the rest of the session."""
import json
import os
import subprocess
import sys
import textwrap

import pytest

from scene_net_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MIN, INT_MAX = -2**31, 2**31 - 1
SN_OK, SN_ERR_INVALID_ARG = 0, -1

# name: (default, variable, what the variable gives when its first character is '1', lo, hi).  lo is None: a switch, which
# stores any value != 0 as 1.  hi is None: no upper bound.
OPTIONS = {
    "conv_skip_empty_tiles": (0, None, None, None, None),
    "conv_i8_tolerance_ppb": (90000, None, None, 0, None),
    "conv_i8_fold": (1, "SN_CONV_I8_NOFOLD", 0, None, None),
    "conv_i8_legacy": (0, "SN_CONV_I8_LEGACY", 1, None, None),
    "conv_i8_no_stage": (0, "SN_CONV_I8_NO_STAGE", 1, None, None),
    "conv_i8z_variant": (2, None, None, 0, 2),
    "conv_no_i8": (0, "SN_CONV_NO_I8", 1, None, None),
    "conv_double_buffer": (0, "SN_CONV_DOUBLE_BUFFER", 1, None, None),
    "conv_lin_no24": (0, "SN_CONV_LIN_NO24", 1, None, None),
    "voxel_onepass": (1, None, None, None, None),
    "voxel_onepass_spin": (64, None, None, 0, None),
    "corr_dense": (0, "SN_CORR_DENSE", 1, None, None),
    "corr_sparse_tile_bytes": (0, None, None, 0, 2048),
    "conv_i8z_inject_fault": (0, None, None, None, None),
}
DEFAULTS = {n: spec[0] for n, spec in OPTIONS.items()}
VARIABLES = {spec[1]: n for n, spec in OPTIONS.items() if spec[1]}
SWITCHES = [n for n, spec in OPTIONS.items() if spec[3] is None]
RANGED = [n for n, spec in OPTIONS.items() if spec[3] is not None]

# the library alone, through ctypes (no torch)
_LIB = """
import ctypes, json, os, sys
lib = ctypes.CDLL(sys.argv[1])
lib.sn_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int]
lib.sn_get_option.argtypes = [ctypes.c_char_p]
lib.sn_last_error.restype = ctypes.c_char_p
def put(name, value):
    return lib.sn_set_option(None if name is None else name.encode(), value)
def get(name):
    return lib.sn_get_option(None if name is None else name.encode())
def error():
    return lib.sn_last_error().decode()
NAMES = json.loads(sys.argv[2])
def everything():
    return {n: get(n) for n in NAMES}
"""
# the Python binding
_BINDING = """
import json, os, sys
sys.path.insert(0, sys.argv[3])
from scene_net_amd import _hip
NAMES = json.loads(sys.argv[2])
def everything():
    return {n: _hip.get_option(n) for n in NAMES}
"""


def _child(body, env=None, prelude=_LIB):
    """Runs `prelude` + `body` in a fresh interpreter whose environment holds none of the option variables but `env`; the
    body prints one JSON value, which is returned."""
    child_env = {k: v for k, v in os.environ.items() if k not in VARIABLES}
    child_env.update(env or {})
    p = subprocess.run([sys.executable, "-c", prelude + textwrap.dedent(body), _hip.LIB_PATH, json.dumps(list(OPTIONS)),
                        ROOT], env=child_env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


# ------------------------------------------------------------------------------------------------------- the library
def test_every_default():
    assert _child("print(json.dumps(everything()))") == DEFAULTS


@pytest.mark.parametrize("name", SWITCHES)
def test_switch_round_trip(name):
    got = _child(f"""
        seen = []
        for v in (1, 0, 5, 0, -3, {INT_MAX}, 0, 1):
            seen.append((put({name!r}, v), get({name!r})))
        print(json.dumps(seen))""")
    assert got == [[SN_OK, v] for v in (1, 0, 1, 0, 1, 1, 0, 1)]


@pytest.mark.parametrize("name", RANGED)
def test_range_bounds(name):
    _, _, _, lo, hi = OPTIONS[name]
    top = INT_MAX if hi is None else hi
    accepted = [lo, lo + 1, top, lo]
    refused = [lo - 1, INT_MIN] + ([] if hi is None else [hi + 1, INT_MAX])
    seen, after = _child(f"""
        seen = [(put({name!r}, v), get({name!r})) for v in {accepted!r}]
        seen += [(put({name!r}, v), get({name!r}), error()) for v in {refused!r}]
        print(json.dumps([seen, everything()]))""")
    assert len(seen) == len(accepted) + len(refused)
    assert seen[:len(accepted)] == [[SN_OK, v] for v in accepted]
    for v, (rc, value, text) in zip(refused, seen[len(accepted):]):
        assert rc == SN_ERR_INVALID_ARG and value == lo, (v, rc, value)   # a refused value changes nothing
        assert name in text, text
    assert after == dict(DEFAULTS, **{name: lo})


def test_null_and_unknown_names():
    got = _child("""
        seen = {"set_null": put(None, 1), "get_null": get(None)}
        for name in ("no_such_option", "conv_i8", "conv_i8_fold_", "CONV_I8_FOLD", ""):
            seen[name] = (put(name, 1), error(), get(name))
        seen["after"] = everything()
        print(json.dumps(seen))""")
    assert got.pop("set_null") == SN_ERR_INVALID_ARG and got.pop("get_null") == -1
    assert got.pop("after") == DEFAULTS
    for name, (rc, text, value) in got.items():
        assert rc == SN_ERR_INVALID_ARG and value == -1, name
        assert f"unknown option '{name}'" in text, text


@pytest.mark.parametrize("given", ["1", "0", "10", "01", "", "yes"])
@pytest.mark.parametrize("variable", sorted(VARIABLES))
def test_variable_sets_its_option(variable, given):
    """only the first character counts: '1' gives the option its variable's value, anything else leaves the default"""
    name = VARIABLES[variable]
    want = dict(DEFAULTS)
    if given[:1] == "1":
        want[name] = OPTIONS[name][2]
    assert _child("print(json.dumps(everything()))", env={variable: given}) == want


@pytest.mark.parametrize("variable", sorted(VARIABLES))
def test_variable_is_read_at_the_first_look_and_never_again(variable):
    name = VARIABLES[variable]
    got = _child(f"""
        os.environ[{variable!r}] = "1"      # after the library loaded, before the first look
        first = get({name!r})
        os.environ[{variable!r}] = "0"
        print(json.dumps([first, get({name!r})]))""")
    assert got == [OPTIONS[name][2]] * 2


@pytest.mark.parametrize("variable", sorted(VARIABLES))
def test_set_before_the_first_look_beats_the_variable(variable):
    name = VARIABLES[variable]
    default = DEFAULTS[name]
    got = _child(f"""
        rc = put({name!r}, {default})
        print(json.dumps([rc, get({name!r}), everything()]))""", env={variable: "1"})
    assert got == [SN_OK, default, DEFAULTS]


# ------------------------------------------------------------------------------------------------------- _hip.options
def test_options_restores_what_it_found_on_a_normal_exit():
    got = _child("""
        _hip.set_option("conv_i8_tolerance_ppb", 1234)   # not the default: what was there is put back, not a constant
        with _hip.options(conv_i8_tolerance_ppb=5, corr_dense=1, conv_i8_fold=0):
            inside = everything()
        print(json.dumps([inside, everything()]))""", prelude=_BINDING)
    inside, after = got
    assert inside == dict(DEFAULTS, conv_i8_tolerance_ppb=5, corr_dense=1, conv_i8_fold=0)
    assert after == dict(DEFAULTS, conv_i8_tolerance_ppb=1234)


def test_options_restores_on_an_exception():
    got = _child("""
        seen = []
        try:
            with _hip.options(conv_i8z_variant=0, voxel_onepass=0):
                seen.append(everything())
                raise KeyError("body")
        except KeyError:
            seen.append(everything())
        try:   # a value out of range: the options set before it are put back too
            with _hip.options(corr_dense=1, corr_sparse_tile_bytes=4096):
                seen.append("body ran")
        except _hip.HipLibraryError as e:
            seen.append(str(e))
        seen.append(everything())
        print(json.dumps(seen))""", prelude=_BINDING)
    inside, after, error, after_refused = got
    assert inside == dict(DEFAULTS, conv_i8z_variant=0, voxel_onepass=0)
    assert after == DEFAULTS
    assert "corr_sparse_tile_bytes" in error
    assert after_refused == DEFAULTS


def test_options_refuses_an_unknown_name_before_changing_anything():
    got = _child("""
        calls, set_option = [], _hip.set_option
        _hip.set_option = lambda name, value: (calls.append(name), set_option(name, value))
        try:
            with _hip.options(corr_dense=1, no_such_option=1):
                print(json.dumps("body ran"))
        except _hip.HipLibraryError as e:
            print(json.dumps([str(e), calls, everything()]))""", prelude=_BINDING)
    error, calls, after = got
    assert "unknown option 'no_such_option'" in error
    assert calls == [] and after == DEFAULTS


def test_options_puts_back_a_value_the_environment_gave():
    got = _child("""
        with _hip.options(conv_i8_legacy=0, conv_i8_fold=1):
            inside = everything()
        print(json.dumps([inside, everything()]))""", env={"SN_CONV_I8_LEGACY": "1", "SN_CONV_I8_NOFOLD": "1"},
                 prelude=_BINDING)
    inside, after = got
    assert inside == DEFAULTS
    assert after == dict(DEFAULTS, conv_i8_legacy=1, conv_i8_fold=0)
