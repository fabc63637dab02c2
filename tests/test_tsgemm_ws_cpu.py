"""CPU-only: the A/B switch of the tall-skinny GEMM and its tile-height query answer without a device."""


def test_tsgemm_variant_switch_and_tile_rows():
    from bevformer_tensorrt_amd.utils import load_library
    lib = load_library()
    assert lib.bevops_tsgemm_set_variant(1) == 0 and lib.bevops_tsgemm_set_variant(0) == 1     # returns the previous value
    new = lib.bevops_tsgemm_tile_rows(256)
    assert new > 0 and new % 32 == 0 and lib.bevops_tsgemm_tile_rows(64) == new
    assert lib.bevops_tsgemm_tile_rows(96) == 0 and lib.bevops_tsgemm_tile_rows(0) == 0
    old = lib.bevops_tsgemm_tile_rows(512)                                                      # K > 256: the original kernel
    assert old > 0 and old % 32 == 0
    prev = lib.bevops_tsgemm_set_variant(1)
    try:
        assert lib.bevops_tsgemm_tile_rows(256) == old
    finally:
        lib.bevops_tsgemm_set_variant(prev)
    assert lib.bevops_query(b"bevops_tsgemm_tile_rows")
