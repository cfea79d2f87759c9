"""kp_cluster_interruptions on the host: what kp_interruptions_validate refuses (no context, nothing runs) and the sizes
of the new structs against the C header (CPU only)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from kpamd import abi

HDR_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
SPOT, CHANGE = abi.MSG_SPOT_INTERRUPTED, abi.MSG_SCHEDULED_CHANGE
MESSAGES = [(SPOT, ["i-1"]), (CHANGE, ["i-2", "i-3", "i-2"]), (abi.MSG_NO_OP, []), (abi.MSG_INSTANCE_TERMINATED, ["i-9"])]
NODE_IDS = ["i-1", None, "i-2", "i-2", "i-3"]


def make(messages=MESSAGES, node_ids=NODE_IDS, table_log2=0, **kw):
    arena = abi.Arena()
    ii = abi.build_interrupt_in(arena, messages, node_ids, table_log2)
    for k, v in kw.items():
        setattr(ii, k, v)
    return arena, ii


def refused(lib, ii, code, text):
    assert lib.kp_interruptions_validate(C.byref(ii)) == code
    assert text in lib.kp_last_error(), lib.kp_last_error()


def test_valid_batches_pass(lib):
    _, ii = make()
    assert lib.kp_interruptions_validate(C.byref(ii)) == 0
    _, ii = make([], [])
    assert lib.kp_interruptions_validate(C.byref(ii)) == 0
    _, ii = make([], [], id_offsets=None)           # no messages: the offsets may be absent
    assert lib.kp_interruptions_validate(C.byref(ii)) == 0
    _, ii = make([(abi.MSG_NO_OP, [])] * 3, [None, None])
    assert lib.kp_interruptions_validate(C.byref(ii)) == 0
    assert lib.kp_abi_version() == 13                # the ABI grew, nothing in it changed


def test_a_null_argument(lib):
    assert lib.kp_interruptions_validate(None) == abi.KP_E_INVAL


@pytest.mark.parametrize("field,text", [("kinds", b"null kinds"), ("id_offsets", b"null kinds or id_offsets"),
                                        ("ids", b"null ids"), ("node_ids", b"null node_ids")])
def test_a_null_array_with_a_count(lib, field, text):
    _, ii = make()
    setattr(ii, field, None)
    refused(lib, ii, abi.KP_E_INVAL, text)


def test_a_null_array_with_a_zero_count_passes(lib):
    _, ii = make([(abi.MSG_NO_OP, [])], [], ids=None)
    assert not ii.node_ids and not ii.ids
    assert lib.kp_interruptions_validate(C.byref(ii)) == 0


def test_a_null_id(lib):
    _, ii = make()
    ii.ids[2] = None
    refused(lib, ii, abi.KP_E_INVAL, b"id 2 is null")


@pytest.mark.parametrize("kind", [-1, 6, 99])
def test_a_kind_outside_the_enum(lib, kind):
    _, ii = make()
    ii.kinds[1] = kind
    refused(lib, ii, abi.KP_E_INVAL, b"message 1: kind")


def test_offsets_that_decrease_or_start_or_end_elsewhere(lib):
    _, ii = make()
    ii.id_offsets[2] = 0
    refused(lib, ii, abi.KP_E_INVAL, b"decrease at message 1")
    _, ii = make()
    ii.id_offsets[0] = 1
    refused(lib, ii, abi.KP_E_INVAL, b"start at 1")
    _, ii = make()
    ii.id_offsets[4] = 3
    refused(lib, ii, abi.KP_E_INVAL, b"decrease at message 3")
    _, ii = make()
    ii.id_offsets[4] = 4
    refused(lib, ii, abi.KP_E_INVAL, b"end at 4 of 5 ids")
    _, ii = make(n_ids=4)
    refused(lib, ii, abi.KP_E_INVAL, b"end at 5 of 4 ids")
    _, ii = make(n_ids=6)
    refused(lib, ii, abi.KP_E_INVAL, b"end at 5 of 6 ids")
    keep, other = make()
    _, ii = make([], [], id_offsets=None, n_ids=1, ids=other.ids)
    refused(lib, ii, abi.KP_E_INVAL, b"end at 0 of 1 ids")


def test_an_id_longer_than_31_bytes_is_unsupported(lib):
    ok, long_id = "i-" + "a" * 29, "i-" + "a" * 30
    _, ii = make([(SPOT, [ok])], [ok])
    assert lib.kp_interruptions_validate(C.byref(ii)) == 0
    _, ii = make([(SPOT, [long_id])], [ok])
    refused(lib, ii, abi.KP_E_UNSUPPORTED, b"id 0 is longer than 31 bytes")
    _, ii = make([(SPOT, [ok])], [ok, None, long_id])
    refused(lib, ii, abi.KP_E_UNSUPPORTED, b"node 2: an instance id longer than 31 bytes")


def test_two_to_the_31_messages_or_ids_is_unsupported_before_any_array_is_read(lib):
    _, ii = make(n_messages=1 << 31)
    refused(lib, ii, abi.KP_E_UNSUPPORTED, b"messages")
    _, ii = make(n_ids=1 << 31)
    refused(lib, ii, abi.KP_E_UNSUPPORTED, b"ids")
    _, ii = make(n_ids=(1 << 31), ids=None, kinds=None)
    refused(lib, ii, abi.KP_E_UNSUPPORTED, b"ids")


def test_a_forced_table_must_exceed_the_nodes_with_an_id(lib):
    _, ii = make(table_log2=3)                        # 8 slots for 4 nodes with an id
    assert lib.kp_interruptions_validate(C.byref(ii)) == 0
    _, ii = make(table_log2=2)                        # 4 slots: none would stay empty
    refused(lib, ii, abi.KP_E_INVAL, b"a forced table of 4 slots for 4 nodes with an id")
    _, ii = make(node_ids=["i-1", None, None], table_log2=1)
    assert lib.kp_interruptions_validate(C.byref(ii)) == 0
    _, ii = make(table_log2=31)
    refused(lib, ii, abi.KP_E_INVAL, b"table_log2 31")


def test_struct_sizes_match_the_c_header(tmp_path):
    """The ctypes and numpy mirrors of kp_cluster_interruptions' structs have the sizes gcc gives the header's, compiled
    as C."""
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    pairs = {"kp_interrupt_node": abi.InterruptNode, "kp_interrupt_delete": abi.InterruptDelete,
             "kp_interrupt_mark": abi.InterruptMark, "kp_interrupt_in": abi.InterruptIn}
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "kp/kp_abi.h"\nint main(void){\n' +
                   "".join(f'printf("%zu\\n", sizeof({k}));\n' for k in pairs) +
                   'printf("%d %d %d\\n", (int)KP_MSG_NO_OP, (int)KP_MSG_INSTANCE_TERMINATED, KP_MESSAGE_KIND_COUNT);\n'
                   "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", HDR_DIR, str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:4] == [C.sizeof(t) for t in pairs.values()], dict(zip(pairs, got))
    assert got[4:] == [abi.MSG_NO_OP, abi.MSG_INSTANCE_TERMINATED, abi.MESSAGE_KIND_COUNT]
    assert C.sizeof(abi.InterruptNode) == abi.interrupt_node_dtype().itemsize == 16
    assert C.sizeof(abi.InterruptDelete) == abi.interrupt_delete_dtype().itemsize == 16
    assert C.sizeof(abi.InterruptMark) == abi.interrupt_mark_dtype().itemsize == 8
    assert C.sizeof(abi.InterruptIn) == 48
    for t, d in ((abi.InterruptNode, abi.interrupt_node_dtype()), (abi.InterruptDelete, abi.interrupt_delete_dtype()),
                 (abi.InterruptMark, abi.interrupt_mark_dtype())):
        assert [f for f, _ in t._fields_] == list(d.names)
