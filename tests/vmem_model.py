"""An independent model of the vmem diagnostic's ops, written from the instructions' definitions with ``struct`` and
``int.from_bytes`` (nothing of csrc/vmem/vmem_ref.h): what a load leaves in the destination registers and what a
store leaves in memory.  tests/test_vmem_cpu.py holds vmem_ref.h against it, tests/test_gpu_vmem.py the device."""
import struct

DWORDS = {"dword": 1, "dwordx2": 2, "dwordx3": 3, "dwordx4": 4}
SUFFIXES = ("_saddr_p4092", "_saddr_m4096", "_saddr_m8", "_saddr", "_sc0_sc1", "_sc0", "_sc1", "_nt", "_p4095",
            "_idxen_offen", "_idxen", "_offen_soffset", "_soffset")


def width(op):
    """``("load" | "store", width name)`` of an op name: ``buffer_load_sbyte_d16_hi`` -> ``("load", "sbyte_d16_hi")``."""
    kind = "store" if "_store_" in op else "load"
    w = op.split(f"_{kind}_", 1)[1]
    more = True
    while more:
        more = False
        for s in SUFFIXES:
            if w.endswith(s):
                w, more = w[:-len(s)], True
    return kind, w


def size(op):
    w = width(op)[1]
    return 4 * DWORDS[w] if w in DWORDS else 2 if "short" in w else 1


def align(op):
    return 16 if op.endswith("_idxen") else min(size(op), 4)


def low(op):
    """The lowest offset ``apply`` takes for the op: its positive immediate needs that much room below the access."""
    return 4096 if op.endswith("p4095") else 4092 if op.endswith("p4092") else 0


def room_above(op):
    return 4096 if op.endswith("m4096") else 8 if op.endswith("m8") else 0


def load(op, mem, off, preset):
    """The 4 words ``apply`` returns for one lane: the registers the load wrote, the rest 0."""
    w = width(op)[1]
    if w in DWORDS:
        return list(struct.unpack_from(f"<{DWORDS[w]}I", mem, off)) + [0] * (4 - DWORDS[w])
    if "short" in w:
        v = int.from_bytes(mem[off:off + 2], "little", signed=w.startswith("s"))
    else:
        v = int.from_bytes(mem[off:off + 1], "little", signed=w.startswith("s"))
    if w.endswith("_d16_hi"):
        r = (preset[0] & 0x0000ffff) | ((v & 0xffff) << 16)
    elif w.endswith("_d16"):
        r = (preset[0] & 0xffff0000) | (v & 0xffff)
    else:
        r = v & 0xffffffff
    return [r, 0, 0, 0]


def store(op, mem, off, data):
    """``mem`` (a bytearray) after one lane's store of the data registers."""
    w = width(op)[1]
    if w in DWORDS:
        struct.pack_into(f"<{DWORDS[w]}I", mem, off, *data[:DWORDS[w]])
    elif w == "byte":
        mem[off] = data[0] & 0xff
    elif w == "byte_d16_hi":
        mem[off] = (data[0] >> 16) & 0xff
    elif w == "short":
        struct.pack_into("<H", mem, off, data[0] & 0xffff)
    else:
        assert w == "short_d16_hi", w
        struct.pack_into("<H", mem, off, data[0] >> 16)
