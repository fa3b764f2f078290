"""Which kernels each library carries (CPU only; beside tests/test_abi.py::test_product_library_reads_no_tuning_variables,
which checks the same separation for the tuning variables' names)."""
from sfmx import _lib


def test_product_library_carries_no_diagnostic_kernels():
    """The kernels only a diagnostic route launches are compiled into lib/libsfmx_diag.so alone
    (csrc/match_diag.hip): a kernel's name is registered as a plain string in the host object, so the
    product library's bytes hold none of these names and the diagnostic library's hold all of them."""
    import diag
    names = (b"sift_screen16_kernel", b"sift_screen6w_kernel", b"sift_subset_kernel", b"sift_settle_kernel",
             b"orb_knn2_kernel", b"prep_hamming_kernel")
    product, diagnostic = open(_lib.LIB_PATH, "rb").read(), open(diag.DIAG_PATH, "rb").read()
    for name in names:
        assert name not in product, name
        assert name in diagnostic, name
