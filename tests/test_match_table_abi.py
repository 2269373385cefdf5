"""CPU-side checks of the table-match entry points (include/kmer_match.h:
kmer_match_open_table, kmer_db_kmers): exported, bound, and NULL arguments
refused before any device call."""
import ctypes


def test_table_match_symbols_are_exported_and_bound():
    from kmerjs_amd import _native
    for name in ("kmer_match_open_table", "kmer_db_kmers"):
        assert name in _native.MATCH_EXPORTS and name in _native.EXPORTS
        assert hasattr(_native.LIB, name)


def test_open_table_rejects_null_without_gpu():
    from kmerjs_amd import _native
    out = ctypes.c_void_p()
    assert _native.LIB.kmer_match_open_table(None, None, ctypes.byref(out)) == 2
    assert _native.LIB.kmer_match_open_table(None, None, None) == 2
    assert b"kmer_match_open_table" in _native.LIB.kmer_match_last_error()
    assert not out.value


def test_db_kmers_rejects_null_without_gpu():
    from kmerjs_amd import _native
    buf = ctypes.create_string_buffer(64)
    assert _native.LIB.kmer_db_kmers(None, 0, 1, buf) == 2
    assert _native.LIB.kmer_db_kmers(None, 0, 0, None) == 2
