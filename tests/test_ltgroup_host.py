"""kp_launch_templates on the host: what kp_launch_templates_validate refuses (no context, nothing runs) and the sizes
of the new structs against the C header (CPU only)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from kpamd import abi
from kpamd.model import AMI

HDR_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
ARCH = "kubernetes.io/arch"


def make(amis=None):
    arena = abi.Arena()
    amis = [AMI("ami-1", [(ARCH, "In", ["amd64"])]), AMI("ami-2", [(ARCH, "NotIn", ["amd64"]), (ARCH, "Exists", [])]),
            AMI("ami-3", [])] if amis is None else amis
    arr, n = abi.amis(arena, amis)
    return arena, arr, n


def test_a_valid_list_and_the_empty_list_pass(lib):
    _, arr, n = make()
    assert lib.kp_launch_templates_validate(arr, n) == 0
    assert lib.kp_launch_templates_validate(None, 0) == 0
    assert lib.kp_launch_templates_validate(arr, 0) == 0
    assert lib.kp_abi_version() == 13


def test_a_null_array_with_a_count(lib):
    assert lib.kp_launch_templates_validate(None, 1) == abi.KP_E_INVAL
    assert b"null amis" in lib.kp_last_error()


def test_a_null_ami_id(lib):
    _, arr, n = make()
    arr[1].id = None
    assert lib.kp_launch_templates_validate(arr, n) == abi.KP_E_INVAL
    assert b"AMI 1 has a null id" in lib.kp_last_error()


@pytest.mark.parametrize("op", [-1, 6, 99])
def test_an_unknown_operator(lib, op):
    _, arr, n = make()
    arr[1].requirements.items[1].op = op
    assert lib.kp_launch_templates_validate(arr, n) == abi.KP_E_INVAL
    assert b"operator" in lib.kp_last_error()


def test_null_requirement_items_keys_value_arrays_and_values(lib):
    _, arr, n = make()
    arr[0].requirements.items = None
    assert lib.kp_launch_templates_validate(arr, n) == abi.KP_E_INVAL
    arr[0].requirements.n = 0  # a NULL array with a zero count passes
    assert lib.kp_launch_templates_validate(arr, n) == 0
    _, arr, n = make()
    arr[1].requirements.items[0].key = None
    assert lib.kp_launch_templates_validate(arr, n) == abi.KP_E_INVAL
    _, arr, n = make()
    arr[0].requirements.items[0].values = None
    assert lib.kp_launch_templates_validate(arr, n) == abi.KP_E_INVAL
    _, arr, n = make()
    arr[0].requirements.items[0].values[0] = None
    assert lib.kp_launch_templates_validate(arr, n) == abi.KP_E_INVAL


def test_more_than_65535_amis_is_unsupported_before_any_array_is_read(lib):
    _, arr, n = make()
    assert lib.kp_launch_templates_validate(arr, 65536) == abi.KP_E_UNSUPPORTED  # (three entries: none is read)
    assert lib.kp_launch_templates_validate(None, 65536) == abi.KP_E_UNSUPPORTED
    arena = abi.Arena()
    arr, n = abi.amis(arena, [AMI(f"ami-{i}", []) for i in range(65535)])
    assert lib.kp_launch_templates_validate(arr, n) == 0


def test_struct_sizes_match_the_c_header(tmp_path):
    """The ctypes and numpy mirrors of kp_launch_templates' structs have the sizes gcc gives the header's, compiled as C."""
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    pairs = {"kp_lt_result": abi.LtResult, "kp_lt_config": abi.LtConfig, "kp_ami": abi.Ami,
             "kp_launch_result": abi.LaunchResult}
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "kp/kp_abi.h"\nint main(void){\n' +
                   "".join(f'printf("%zu\\n", sizeof({k}));\n' for k in pairs) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", HDR_DIR, str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(t) for t in pairs.values()], dict(zip(pairs, got))
    assert C.sizeof(abi.LtResult) == abi.lt_result_dtype().itemsize == 16
    assert C.sizeof(abi.LtConfig) == abi.lt_config_dtype().itemsize == 32
    assert [f for f, _ in abi.LtConfig._fields_] == list(abi.lt_config_dtype().names)
    assert [f for f, _ in abi.LtResult._fields_] == list(abi.lt_result_dtype().names)
