"""The zstd encoder's host-side surface, without a GPU: the output bound, argument checks of the batch entry point, and the Rust
glue's constructor."""
import os

from conftest import ROOT

FMT_ZSTD = 100


def test_encode_bound_covers_raw_blocks_header_and_checksum():
    import compu_amd

    for n in [0, 1, 2, 100, 65535, 131071, 131072, 131073, 262144, 1 << 20, (1 << 20) + 1, 5_000_000, (1 << 27) + 5, 0xFFFFFFF0]:
        blocks = max(1, -(-n // (128 << 10)))
        assert compu_amd.encode_bound(FMT_ZSTD, n) >= n + 3 * blocks + 18 + 4, n


def test_batch_rejects_out_of_range_level_and_strategy():
    import ctypes as C

    import compu_amd

    L = compu_amd.lib()
    one = C.c_void_p(8)  # never dereferenced: the arguments are checked first
    for level, strategy in ((131073, 0), (-131073, 0), (3, 10), (3, -1)):
        rc = L.chip_encode_batch_ex(FMT_ZSTD, level, strategy, 1, one, one, one, one, one, one, one, one, None)
        assert rc == -101, (level, strategy, rc)


def test_rust_glue_defines_zstd_hip():
    src = open(os.path.join(ROOT, "integration", "src", "encoder", "hip.rs")).read()
    assert "pub fn zstd_hip(opts: ZstdOptions) -> Option<Encoder>" in src
    assert "static HIP_ZSTD: Interface" in src
    assert "chip_encoder_new_zstd" in open(os.path.join(ROOT, "integration", "src", "hip_sys.rs")).read()
