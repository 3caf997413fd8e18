"""Writes tests/golden/lz4/: both golden texts as raw LZ4 blocks (LZ4_compress_default, LZ4_compress_HC at level 9) and as frames
(LZ4F_compressFrame with default preferences -- linked 64 KiB blocks, no checksums -- and with independent blocks, block
checksums, content size and content checksum), made with the system's liblz4.  The fixtures are committed; this only says how
they were made.  liblz4 1.9.3 wrote the committed ones."""
import ctypes as C
import ctypes.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FrameInfo(C.Structure):
    _fields_ = [("blockSizeID", C.c_int), ("blockMode", C.c_int), ("contentChecksumFlag", C.c_int), ("frameType", C.c_int),
                ("contentSize", C.c_ulonglong), ("dictID", C.c_uint), ("blockChecksumFlag", C.c_int)]


class Preferences(C.Structure):
    _fields_ = [("frameInfo", FrameInfo), ("compressionLevel", C.c_int), ("autoFlush", C.c_uint), ("favorDecSpeed", C.c_uint),
                ("reserved", C.c_uint * 3)]


def main():
    lz4 = C.CDLL(ctypes.util.find_library("lz4"))
    lz4.LZ4F_compressFrameBound.restype = C.c_size_t
    lz4.LZ4F_compressFrameBound.argtypes = [C.c_size_t, C.c_void_p]
    lz4.LZ4F_compressFrame.restype = C.c_size_t
    lz4.LZ4F_compressFrame.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    out_dir = os.path.join(ROOT, "tests", "golden", "lz4")
    os.makedirs(out_dir, exist_ok=True)
    for name in ("10x10y", "alice29.txt"):
        data = open(os.path.join(ROOT, "tests", "golden", name), "rb").read()
        room = C.create_string_buffer(lz4.LZ4_compressBound(len(data)))
        n = lz4.LZ4_compress_default(data, room, len(data), len(room))
        assert n > 0
        open(os.path.join(out_dir, name + ".default.block"), "wb").write(room.raw[:n])
        n = lz4.LZ4_compress_HC(data, room, len(data), len(room), 9)
        assert n > 0
        open(os.path.join(out_dir, name + ".hc.block"), "wb").write(room.raw[:n])
        full = Preferences()
        full.frameInfo.blockSizeID, full.frameInfo.blockMode, full.frameInfo.contentChecksumFlag = 4, 1, 1
        full.frameInfo.contentSize, full.frameInfo.blockChecksumFlag = len(data), 1
        for tag, prefs in (("default", None), ("full", C.byref(full))):
            room = C.create_string_buffer(lz4.LZ4F_compressFrameBound(len(data), prefs))
            n = lz4.LZ4F_compressFrame(room, len(room), data, len(data), prefs)
            assert n < (1 << 40), "LZ4F error"
            open(os.path.join(out_dir, name + "." + tag + ".lz4"), "wb").write(room.raw[:n])
    print(sorted(os.listdir(out_dir)))


if __name__ == "__main__":
    main()
