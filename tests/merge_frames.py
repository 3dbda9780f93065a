"""Hand-built PARTIAL rows for the merge tests: the saved states (results.cc save_state) and
SValue::encode (svalue.cc:311-315) of a row's cells, and a walk of a frame payload in python."""
import struct

from eventql_amd import capi as K
import oracle_lib as O


def st_uint(v):
    """count / integer sum"""
    return O.varuint(v & (2 ** 64 - 1))


def st_f64(x):
    """sum(float64)"""
    return struct.pack("<d", x)


def st_cnt_f64(cnt, x):
    """min / max / mean over floats (mean: the float sum)"""
    return O.varuint(cnt) + struct.pack("<d", x)


def st_cnt_u64(cnt, v):
    return O.varuint(cnt) + struct.pack("<Q", v & (2 ** 64 - 1))


def sv(stype, body):
    return bytes([stype]) + O.varuint(len(body)) + body


def sv_u64(v, tag=0):
    return sv(K.T_UINT64, struct.pack("<Q", v) + bytes([tag]))


def sv_f64(x, tag=0):
    return sv(K.T_FLOAT64, struct.pack("<d", x) + bytes([tag]))


def sv_str(s, tag=0):
    return sv(K.T_STRING, struct.pack("<I", len(s)) + s + bytes([tag]))


def sv_nil():
    return sv(K.T_NIL, b"")


def key(i):
    """a 20-byte key whose first 8 bytes differ from every other i's"""
    return struct.pack("<QQI", (i * 0x9E3779B97F4A7C15 + 1) & (2 ** 64 - 1), i, 7)


def read_varuint(buf, pos):
    v = shift = 0
    while True:
        b = buf[pos]
        pos += 1
        v |= (b & 0x7f) << shift
        shift += 7
        if not b & 0x80:
            return v, pos


def walk_frame(payload, cells):
    """row offsets (rows + 1) of a frame payload; cells: per select expression 'u' (varuint
    state), 'f' (8 raw bytes), 'c' (varuint count + 8 bytes) or 's' (an SValue)"""
    _flags, pos = read_varuint(payload, 0)
    count, pos = read_varuint(payload, pos)
    off = []
    for _ in range(count):
        off.append(pos)
        pos += 20
        for c in cells:
            if c == "u":
                _, pos = read_varuint(payload, pos)
            elif c == "f":
                pos += 8
            elif c == "c":
                _, pos = read_varuint(payload, pos)
                pos += 8
            else:
                n, pos = read_varuint(payload, pos + 1)
                pos += n
    off.append(pos)
    return off
