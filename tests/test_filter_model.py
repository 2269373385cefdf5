"""The Python model of the read filter (tests/filter_util.py), which the GPU
tests take their expected bytes from, against literal expected bytes: record
splitting on the edge inputs, the predicate, pairing and DROP."""
import pytest

from tests.filter_util import EDGE_INPUTS, FILTER_DROP, FILTER_PAIRED, filter_model, keep_flags, match, split_records

A, B, C = b"@a\nACGTA\n+\nIIIII\n", b"@b\nGG\n+\nII\n", b"@c\nTTT\n+\nIII\n"

RECORDS = {
    "empty": [],
    "no_newline": [],
    "nl1": [b"@a\n"],
    "nl2": [b"@a\nACGTA\n"],
    "nl3": [b"@a\nACGTA\n+\n"],
    "nl4": [A],
    "nl5": [A, b"@b\n"],
    "nl8": [A, B],
    "partial_header": [A, B],
    "no_final_newline": [A, b"@b\nGG\n+\nII"],
    "crlf": [b"@a\r\nACGTA\r\n+\r\nIIIII\r\n", b"@b\r\nGG\r\n+\r\nII\r\n"],
    "three": [A, B, C],
}


@pytest.mark.parametrize("name", sorted(EDGE_INPUTS))
def test_records_of_the_edge_inputs(name):
    data, n, consumed = EDGE_INPUTS[name]
    recs = split_records(data)
    assert recs == RECORDS[name]
    assert len(recs) == n == len(data.split(b"\n")[1::4])
    assert b"".join(recs) == data[:consumed]
    assert b"\n" not in data[consumed:] or n == 0
    # identity and emptiness: min_hits 0 and frac 0/1 keep every read, also one without windows
    rows = [(0, 0)] * n
    out, keep, res = filter_model(data, rows, 0, (0, 1), 0)
    assert out == data[:consumed] and keep == [True] * n
    assert res == {"n_reads": n, "n_kept": n, "out_len": consumed, "consumed": consumed}
    out, keep, res = filter_model(data, rows, 0, (0, 1), FILTER_DROP)
    assert out == b"" and keep == [False] * n
    assert res == {"n_reads": n, "n_kept": 0, "out_len": 0, "consumed": consumed}


def test_the_tails():
    assert EDGE_INPUTS["partial_header"][0][28:] == b"@c part"
    assert EDGE_INPUTS["no_newline"][0][0:] == b"@r0 ACGT"
    assert EDGE_INPUTS["no_final_newline"][2] == len(EDGE_INPUTS["no_final_newline"][0])


def test_predicate():
    assert match(0, 0, 0, (0, 1)) and not match(0, 0, 1, (0, 1))
    assert match(10, 5, 1, (1, 2)) and not match(11, 5, 1, (1, 2)) and match(11, 6, 1, (1, 2))
    assert not match(10, 5, 6, (0, 1)) and match(10, 5, 5, (0, 1))
    assert match(3, 2, 1, (2, 3)) and not match(3, 1, 1, (2, 3)) and match(0, 0, 0, (1, 1))
    big = (1 << 64) - 1
    assert match(big, big, big, ((1 << 32) - 1, (1 << 32) - 1)) and not match(big, big - 1, 0, (1, 1))


def test_keep_and_drop_give_literal_bytes():
    data = EDGE_INPUTS["three"][0]
    rows = [(5, 5), (2, 0), (3, 2)]
    assert filter_model(data, rows, 1)[0] == A + C
    assert filter_model(data, rows, 1, flags=FILTER_DROP)[0] == B
    assert filter_model(data, rows, 1, (1, 1))[0] == A
    assert filter_model(data, rows, 1, (2, 3))[:2] == (A + C, [True, False, True])
    assert filter_model(data, rows, 3)[0] == A
    out, keep, res = filter_model(data + b"@tail", rows, 1)
    assert out == A + C and res == {"n_reads": 3, "n_kept": 2, "out_len": 30, "consumed": 41}
    # the input's last record without its final '\n' is last in the output too
    out, keep, res = filter_model(data[:-1], rows, 1)
    assert out == A + C[:-1] and res["consumed"] == 40


def test_crlf_records_are_kept_verbatim():
    data = EDGE_INPUTS["crlf"][0]
    assert filter_model(data, [(0, 0), (1, 1)], 1)[0] == b"@b\r\nGG\r\n+\r\nII\r\n"


def test_paired_with_an_odd_record_count():
    data = EDGE_INPUTS["three"][0]
    P = FILTER_PAIRED
    assert keep_flags([(5, 5), (2, 0), (3, 0)], 1, (0, 1), P) == [True, True, False]     # first mate only
    assert keep_flags([(5, 0), (2, 2), (3, 0)], 1, (0, 1), P) == [True, True, False]     # second mate only
    assert keep_flags([(5, 0), (2, 0), (3, 3)], 1, (0, 1), P) == [False, False, True]    # the last one, judged alone
    assert filter_model(data, [(5, 0), (2, 2), (3, 0)], 1, flags=P)[0] == A + B
    assert filter_model(data, [(5, 0), (2, 2), (3, 0)], 1, flags=P | FILTER_DROP)[0] == C
    assert filter_model(data, [(5, 0), (2, 0), (3, 3)], 1, flags=P | FILTER_DROP)[0] == A + B
    assert keep_flags([(5, 5), (2, 0), (3, 0), (1, 1)], 1, (0, 1), P) == [True] * 4
