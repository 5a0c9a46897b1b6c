"""Guard zones of the engine's device arrays (csrc/device_guards.hpp) without a GPU: a stand-alone C++ program includes the header alone,
lays a payload between two zones in host memory the way DeviceOwner::device_bytes lays it out on the device, damages known bytes and
prints what guard_scan reports.  The expected values are worked out by hand from the layout: zone | payload | zone, the back zone
beginning at the payload's end to the byte.  The same program is built and run a second time under AddressSanitizer and UBSan (a host
program with its own main: nothing is preloaded), so that the scan itself is known not to read outside the two zones."""
import os
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ZONE = 256
# name: (payload bytes, [(offset from the allocation's start, bytes written)]) -> (total, payload offset, back offset, before count, before first, behind count, behind first)
CASES = {
    "clean": ((100, []), (612, 256, 356, 0, 0, 0, 0)),
    "one byte before the payload": ((100, [(255, 1)]), (612, 256, 356, 1, 1, 0, 0)),
    "bytes behind it": ((100, [(356 + 4, 4)]), (612, 256, 356, 0, 0, 4, 4)),
    "the byte right behind an odd-sized payload": ((101, [(357, 1)]), (613, 256, 357, 0, 0, 1, 0)),
    "both sides": ((100, [(200, 8), (356, 12)]), (612, 256, 356, 8, 49, 12, 0)),
    "the first byte of the front zone": ((100, [(0, 1)]), (612, 256, 356, 1, 256, 0, 0)),
    "the last byte of the back zone": ((100, [(611, 1)]), (612, 256, 356, 0, 0, 1, 255)),
    "a payload of 0 bytes, clean": ((0, []), (512, 256, 256, 0, 0, 0, 0)),
    "a payload of 0 bytes, a store at its address": ((0, [(256, 4)]), (512, 256, 256, 0, 0, 4, 0)),
    "the payload itself is not looked at": ((100, [(256, 100)]), (612, 256, 356, 0, 0, 0, 0)),
}
# zone sizes v2p_debug_guards accepts (0 = off) and refuses
ZONES_OK = [0, 256, 4096, 1 << 20]
ZONES_BAD = [-256, 1, 100, 255, 257, 4097, (1 << 20) + 256]

PROG = r'''
#include "device_guards.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int main(int argc, char** argv) {
    if (argc == 2) {  // zone size -> accepted?
        printf("%d\n", (int)v2p::guard_zone_valid(atoll(argv[1])));
        return 0;
    }
    // zone bytes [offset count]...
    const size_t zone = (size_t)atoll(argv[1]), bytes = (size_t)atoll(argv[2]);
    const v2p::GuardLayout lay = v2p::guard_layout(bytes, zone);
    unsigned char* base = (unsigned char*)malloc(lay.total);  // (exactly the allocation's size: the sanitizer build sees a scan that leaves it)
    memset(base, v2p::GUARD_BYTE, zone);
    memset(base + lay.payload, 0x11, bytes);
    memset(base + lay.back, v2p::GUARD_BYTE, zone);
    for (int k = 3; k + 1 < argc; k += 2) memset(base + atoll(argv[k]), 0, (size_t)atoll(argv[k + 1]));
    // what check_guards does: a host copy of the two zones, front first
    unsigned char* host = (unsigned char*)malloc(2 * zone);
    memcpy(host, base, zone);
    memcpy(host + zone, base + lay.payload + bytes, zone);
    const v2p::GuardScan s = v2p::guard_scan(host, host + zone, zone);
    printf("%zu %zu %zu %zu %zu %zu %zu %d\n", lay.total, lay.payload, lay.back, s.before_count, s.before_first, s.behind_count, s.behind_first, (int)s.clean());
    free(host);
    free(base);
    return 0;
}
'''


def _build(d, extra):
    src = os.path.join(d, "s.cpp")
    open(src, "w").write(PROG)
    path = os.path.join(d, "s" + str(len(extra)))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-g"] + extra + ["-I", os.path.join(REPO, "vid2player3d_amd", "csrc"), src, "-o", path])
    return path


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request):
    with tempfile.TemporaryDirectory() as d:
        yield _build(d, [] if request.param == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def run(exe, args):
    return [int(x) for x in subprocess.check_output([exe] + [str(a) for a in args]).split()]


@pytest.mark.parametrize("name", list(CASES))
def test_guard_scan(exe, name):
    (bytes_, writes), want = CASES[name]
    got = run(exe, [ZONE, bytes_] + [x for w in writes for x in w])
    print(name, got)
    assert tuple(got[:7]) == want
    assert got[7] == int(want[3] == 0 and want[5] == 0)


def test_guard_rows_of_the_task_buffers():
    """The Python half (HumanoidSMPLIM._buffer / _check_guard_rows, cfg env debug_guard_rows) on CPU tensors: the slice handed out is the
    contiguous middle of the storage, 64 rows in, every dtype the tasks allocate; a store into a guard row is named with its tensor, its
    side and its row; stores into the payload are not."""
    import types

    import torch

    from vid2player3d_amd.tasks.humanoid_smpl_im import HumanoidSMPLIM

    def stub(rows):
        t = types.SimpleNamespace(_guard_rows=rows, _guarded_buffers=[], device="cpu", GUARD_BYTE=HumanoidSMPLIM.GUARD_BYTE)
        t.B = lambda *a, **k: HumanoidSMPLIM._buffer(t, *a, **k)
        t.check = lambda: HumanoidSMPLIM._check_guard_rows(t)
        return t

    plain = stub(0)
    x = plain.B("x", (5, 3))
    assert x.shape == (5, 3) and x.untyped_storage().nbytes() == 5 * 3 * 4 and not plain._guarded_buffers and (plain.B("r", (5,), torch.long, fill=1) == 1).all()
    t = stub(64)
    bufs = {"f": t.B("f", (5, 461)), "i": t.B("i", (5,), torch.long, fill=1), "u": t.B("u", (5, 7), torch.uint8), "b": t.B("b", (5,), torch.bool),
            "i32": t.B("i32", (5, 2), torch.int32), "links": t.B("links", (5 * 24, 13), rows_per_env=24)}
    for name, v in bufs.items():
        per_env = 24 if name == "links" else 1
        assert v.is_contiguous() and v.shape[0] == 5 * per_env
        offset = v.data_ptr() - v.untyped_storage().data_ptr()
        assert offset == 64 * per_env * v[0].numel() * v.element_size(), name
        assert offset % 256 == 0 or v.element_size() < 4, name
        assert (v == (1 if name == "i" else 0)).all(), name
    full = t._guarded_buffers[1][1]
    assert full[0].item() == 0x5A5A5A5A5A5A5A5A and full[-1].item() == 0x5A5A5A5A5A5A5A5A
    t.check()
    for v in bufs.values():
        v.fill_(1)  # the payload is the caller's
    t.check()
    for name, row, side in (("f", -1, "in front of"), ("f", 5, "behind"), ("i", 5 + 63, "behind"), ("b", -64, "in front of"), ("links", 5 * 24, "behind")):
        full = next(f for n, f, g in t._guarded_buffers if n == name)
        g = next(g for n, f, g in t._guarded_buffers if n == name)
        raw = full.view(torch.uint8) if full.dtype == torch.bool else full  # (a copy between bool tensors would normalise 0x5A to 1)
        keep = raw[g + row].clone()
        raw[g + row] = 0
        with pytest.raises(RuntimeError, match="'%s'.*%s" % (name, side)):
            t.check()
        raw[g + row] = keep
        t.check()


def test_zone_sizes(exe):
    for z in ZONES_OK:
        assert run(exe, [z]) == [1], z
    for z in ZONES_BAD:
        assert run(exe, [z]) == [0], z
