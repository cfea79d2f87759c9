"""kp_catalog_compile on the host: what it refuses with ctx = NULL (validation only, nothing is written) and the sizes of
its structs against the C header (CPU only)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import kpamd
from kpamd import abi, catalog
from kpamd.catalog import CapacityReservation as CR

HDR_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
ROWS = catalog.load_ec2_table()[:3]
NAMES = [r["name"] for r in ROWS]


def make(**kw):
    """(arena, kp_compile_in, kp_compile_out) of a small valid call: 3 types, 2 NodeClasses, the 3 default zones"""
    arena = abi.Arena()
    args = dict(unavailable=[("spot", NAMES[0], catalog.ZONES[0]), "on-demand", catalog.ZONES[1]],
                reservations=[[CR("cr-1", NAMES[1], catalog.ZONES[2], "default", 1)], []],
                discovered_memory={(1, NAMES[2]): 1 << 30})
    args.update(kw)
    cin = kpamd.build_compile_in(arena, catalog.default_options(), ROWS, [dict(), dict(max_pods=20)], catalog.ZONES,
                                 spot_prices=catalog.default_spot_prices(ROWS), **args)
    it_zones = (C.c_uint64 * 6)()
    arena.keep.append(it_zones)
    return arena, cin, abi.CompileOut(it_zones=it_zones)


def run(lib, cin, out):
    return lib.kp_catalog_compile(None, C.byref(cin), C.byref(out), None)


def test_a_valid_call_validates_and_writes_nothing(lib):
    _, cin, out = make()
    out.it_zones[0] = 77
    assert run(lib, cin, out) == 0
    assert out.it_zones[0] == 77
    assert lib.kp_abi_version() == 13


def test_null_in_out_and_all_outputs_null(lib):
    _, cin, out = make()
    assert lib.kp_catalog_compile(None, None, C.byref(out), None) == abi.KP_E_INVAL
    assert lib.kp_catalog_compile(None, C.byref(cin), None, None) == abi.KP_E_INVAL
    assert run(lib, cin, abi.CompileOut()) == abi.KP_E_INVAL
    assert b"every output is NULL" in lib.kp_last_error()


@pytest.mark.parametrize("field", ["types", "nodeclasses", "all_zones", "type_zones", "od_price", "spot_price",
                                   "unavailable", "reservations", "reservation_offsets"])
def test_a_null_array_whose_count_is_not_zero(lib, field):
    _, cin, out = make()
    setattr(cin, field, None)
    assert run(lib, cin, out) == abi.KP_E_INVAL


def test_null_arrays_with_a_zero_count_pass(lib):
    _, cin, out = make()
    cin.unavailable, cin.n_unavailable = None, 0
    cin.reservations, cin.reservation_offsets, cin.n_reservations = None, None, 0
    cin.discovered_memory = None
    assert run(lib, cin, out) == 0


def test_more_than_64_zones_is_unsupported(lib):
    _, cin, out = make()
    cin.n_all_zones = 65  # refused before any array is read
    assert run(lib, cin, out) == abi.KP_E_UNSUPPORTED
    cin.n_all_zones = 3
    assert run(lib, cin, out) == 0


@pytest.mark.parametrize("n_nodeclasses,n_types,n_zones", [(1 << 16, 1 << 15, 1), (2, 1 << 30, 1), (1, 1 << 24, 64),
                                                           (1 << 16, 1, 1)])
def test_products_past_32_bit_indexing_are_unsupported(lib, n_nodeclasses, n_types, n_zones):
    _, cin, out = make()
    cin.n_nodeclasses, cin.n_types, cin.n_all_zones = n_nodeclasses, n_types, n_zones  # refused before any array is read
    assert run(lib, cin, out) == abi.KP_E_UNSUPPORTED


def test_a_negative_price(lib):
    arena, cin, out = make()
    cin.od_price[1] = -0.5
    assert run(lib, cin, out) == abi.KP_E_INVAL
    cin.od_price[1] = float("nan")  # no price
    assert run(lib, cin, out) == 0
    cin.spot_price[2 * 3 + 1] = -1e-9
    assert run(lib, cin, out) == abi.KP_E_INVAL
    cin.spot_price[2 * 3 + 1] = float("inf")
    assert run(lib, cin, out) == 0


def test_a_discovered_memory_that_overflows_milli_units(lib):
    _, cin, out = make()
    cin.discovered_memory[1 * 3 + 2] = (2**63 - 1) // 1000 + 1
    assert run(lib, cin, out) == abi.KP_E_INVAL
    cin.discovered_memory[1 * 3 + 2] = (2**63 - 1) // 1000  # the largest value whose milli-units fit
    assert run(lib, cin, out) == 0


def test_zone_names_and_type_zones(lib):
    _, cin, out = make()
    cin.type_zones[2] = 0b1000
    assert run(lib, cin, out) == abi.KP_E_INVAL
    arena, cin, out = make()
    cin.all_zones[1] = arena.s(catalog.ZONES[0])  # (the arena keeps the interned bytes)
    assert run(lib, cin, out) == abi.KP_E_INVAL
    _, cin, out = make()
    cin.all_zones[2] = None
    assert run(lib, cin, out) == abi.KP_E_INVAL


@pytest.mark.parametrize("entry", [("spot", NAMES[0], "nowhere"), ("reserved", NAMES[0], catalog.ZONES[0]), "nowhere",
                                   abi.Unavailable(b"spot", catalog.ZONES[0].encode(), 3, 0),
                                   abi.Unavailable(b"spot", catalog.ZONES[0].encode(), -1, 0),
                                   abi.Unavailable(b"spot", None, 1, 0), abi.Unavailable(None, catalog.ZONES[0].encode(), 1, 0),
                                   abi.Unavailable(None, None, -1, 0), abi.Unavailable(b"Spot", None, -1, 0)])
def test_an_unavailable_entry_of_no_form_or_naming_something_unknown(lib, entry):
    if isinstance(entry, abi.Unavailable):
        _, cin, out = make()
        cin.unavailable[1] = entry
    else:
        _, cin, out = make(unavailable=[entry])
    assert run(lib, cin, out) == abi.KP_E_INVAL


def test_reservations(lib):
    _, cin, out = make()
    cin.reservations[0].type = 3
    assert run(lib, cin, out) == abi.KP_E_INVAL
    _, cin, out = make()
    cin.reservations[0].zone = b"nowhere"
    assert run(lib, cin, out) == abi.KP_E_INVAL
    _, cin, out = make()
    cin.reservations[0].id = None
    assert run(lib, cin, out) == abi.KP_E_INVAL
    for offsets in ([1, 1, 1], [0, 2, 1], [0, 0, 0]):
        _, cin, out = make()
        for i, v in enumerate(offsets):
            cin.reservation_offsets[i] = v
        assert run(lib, cin, out) == abi.KP_E_INVAL, offsets
    _, cin, out = make()
    cin.reserved_capacity = 0  # the gate being off does not skip the validation
    cin.reservations[0].type = 3
    assert run(lib, cin, out) == abi.KP_E_INVAL


def test_a_nodeclass_with_null_zones_or_block_device_mappings(lib):
    _, cin, out = make()
    cin.nodeclasses[1].zones = None
    assert run(lib, cin, out) == abi.KP_E_INVAL
    _, cin, out = make()
    cin.nodeclasses[0].n_block_device_mappings = 1
    assert run(lib, cin, out) == abi.KP_E_INVAL


def test_struct_sizes_match_the_c_header(tmp_path):
    """The ctypes mirrors of kp_catalog_compile's structs have the sizes gcc gives the header's, compiled as C."""
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    pairs = {"kp_unavailable": abi.Unavailable, "kp_compile_reservation": abi.CompileReservation,
             "kp_reserved_offering": abi.ReservedOffering, "kp_compile_in": abi.CompileIn, "kp_compile_out": abi.CompileOut}
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "kp/kp_abi.h"\nint main(void){\n' +
                   "".join(f'printf("%zu\\n", sizeof({k}));\n' for k in pairs) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", HDR_DIR, str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(t) for t in pairs.values()], dict(zip(pairs, got))
    assert C.sizeof(abi.ReservedOffering) == abi.reserved_offering_dtype().itemsize == 16
    assert C.sizeof(abi.ResourceList) == abi.resource_list_dtype().itemsize
