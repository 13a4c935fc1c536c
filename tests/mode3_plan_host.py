"""Host restatement of the mode-3 tile plan (csrc/cti_mode3_plan.hip, csrc/cti_f16f6.h "tile plan") that the tests compare the device's totals against."""
import numpy as np

BM, BN = 256, 192            # the f16f6 product's tile in the default build (csrc/cti_gemm_f16f6.hip, GeoF6; the library's f6_mode3_tile_rows / _cols).  The
                             # experiment build's CTI_F6_GEO=half geometry (-DCTI_F6_WITH_HALF_GEO, 128-row tiles) is not what these tests describe


def zero_object_mask(v):
    """(B, V) bool: every element of the object's feature row is +-0 -- the bit-exact magnitude OR of cti_zero_row_mask (NaN / inf / subnormals are not zero)."""
    bits = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32) & np.uint32(0x7fffffff)
    return (bits == 0).all(axis=-1)


def live_row_tiles(mask_row, rows_per_obj, bm=BM):
    """Row tiles the product computes for one sample: those that hold its objects up to and including the first object of the TRAILING run of all-zero objects."""
    n_objs = len(mask_row)
    n_rep = n_objs
    while n_rep > 0 and mask_row[n_rep - 1]:
        n_rep -= 1
    return -(-min(n_objs, n_rep + 1) * rows_per_obj // bm), n_rep


def host_plan(mask, Q, G, A, bm=BM, bn=BN):
    """Totals of the plan for a (B, V) mask: tiles walked, row tiles among them, product rows (of V * Q * G per sample) filled by copy."""
    n_objs = mask.shape[1]
    rows = n_objs * Q * G
    tiles_n = -(-A // bn)
    live = [live_row_tiles(m, Q * G, bm)[0] for m in mask]
    return {"live_tiles": sum(live) * tiles_n, "live_row_tiles": sum(live), "filled_rows": sum(max(0, rows - t * bm) for t in live)}
