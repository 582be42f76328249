"""The pool-products ABI without a GPU: the record layout and the argument checks that come before any device work."""
import ctypes as C

import numpy as np

from pcramp_amd import api

PCR_ERR_ARG = -1


def test_product_record_layout():
    dt = api.PRODUCT_DTYPE
    assert dt.itemsize == 32                                                   # sizeof(pcr_product)
    assert dt.names == ("plus_oligo", "minus_oligo", "sequence", "begin", "end", "inner_start", "inner_length", "intended")
    assert [dt.fields[n][1] for n in dt.names] == list(range(0, 32, 4))


def test_pool_products_rejects_bad_arguments():
    L = api.load_library()
    pool = np.zeros((1, 4), np.uint64)
    ids = np.zeros(2, np.uint32)
    out = np.zeros(1, api.PRODUCT_DTYPE)
    # no handle, and a set that is not TARGET or BACKGROUND: refused before any device call
    assert L.pcr_pool_products(None, api.TARGET, pool.ctypes.data, 1, 1.0, 80, 200, ids.ctypes.data, out.ctypes.data, 1) == PCR_ERR_ARG
    assert L.pcr_pool_products(None, 7, pool.ctypes.data, 1, 1.0, 80, 200, ids.ctypes.data, out.ctypes.data, 1) == PCR_ERR_ARG
    assert b"pcr_pool_products" in L.pcr_last_error()
