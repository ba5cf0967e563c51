"""find-unique-kmers step, CPU side: the cut-off rule (the reference's own arithmetic) against
golden vectors recorded from the real reference function, for the oracle and for the product's
host function alike; the oracle's restatement of the KMC steps on hand-checked toy input."""
import io
import contextlib

import pytest

from conftest import load_golden


def _cases():
    return load_golden("unique_cutoffs.json")["cases"]


def test_oracle_cutoffs_match_reference_vectors():
    from oracle import unique_oracle as uo

    n_ok = 0
    for c in _cases():
        rows = [tuple(r) for r in c["histogram"]]
        if "error" in c["expect"]:
            with pytest.raises(uo.HistogramError):
                uo.analyze_histogram_rows(rows)
        else:
            lo, hi, warned = uo.analyze_histogram_rows(rows)
            assert (lo, hi, warned) == (c["expect"]["min"], c["expect"]["max"], c["expect"]["warned"])
            n_ok += 1
    assert n_ok >= 40


def test_product_cutoffs_match_reference_vectors(built):
    from trio_binning_amd import find_unique_kmers as fu

    for c in _cases():
        rows = [tuple(r) for r in c["histogram"]]
        err = io.StringIO()
        with contextlib.redirect_stderr(err):
            if "error" in c["expect"]:
                with pytest.raises(fu.HistogramError) as e:
                    fu.analyze_histogram(rows, "h.txt")
                assert "Could not find min and max counts in histogram" in e.value.message
                continue
            lo, hi = fu.analyze_histogram(rows, "h.txt")
        assert (lo, hi) == (c["expect"]["min"], c["expect"]["max"])
        assert ("WARNING" in err.getvalue()) == c["expect"]["warned"]


def test_oracle_kmc_steps_on_toy_input():
    from oracle import unique_oracle as uo

    k = 3
    reads_a = ["ACGTAC", "acgNAC", "GTACGT"]  # lower case counts, N breaks windows
    counts = uo.count_kmers(reads_a, k)
    # ACG/CGT are each other's reverse complement: canonical ACG; GTA/TAC -> canonical GTA
    assert counts == {"ACG": 5, "GTA": 4}
    db = uo.database(counts)
    assert db == {"ACG": 5, "GTA": 4}
    assert uo.database(uo.count_kmers(["ACGTT"], k)) == {"ACG": 2}  # AAC (from GTT) seen once: not stored
    rows = uo.histogram_rows(db)
    assert rows[0] == (1, 0) and rows[3] == (4, 1) and rows[4] == (5, 1) and len(rows) == 255
    assert uo.database({"AAA": 300, "AAC": 1}) == {"AAA": 255}
    assert uo.unique_kmers(db, {"GTA": 2}, 2, 10) == ["ACG"]
    assert uo.unique_kmers(db, {}, 5, 10) == ["ACG"] and uo.unique_kmers(db, {}, 2, 10) == ["ACG", "GTA"]


def test_oracle_c_counter_equals_python_restatement():
    """The oracle's C counter (checker at scale, CPU datum) against the pure-Python restatement."""
    from collections import Counter

    import numpy as np

    from oracle import binding
    from oracle import unique_oracle as uo

    orc = binding.load()
    rng = np.random.default_rng(1)
    g = "".join("ACGT"[c] for c in rng.integers(0, 4, 3000))
    reads = [g[p:p + 100] for p in rng.integers(0, 2900, 400)] + ["acgtNacgtacgtacgtacgtacgtttt", "", g[:20], "N" * 50]
    bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    for k in (1, 5, 21, 31, 32):
        h = orc.kmer_histogram(bases, offs, k, 100_000)
        c = uo.count_kmers(reads, k)
        want = Counter(min(v, 255) for v in c.values())
        assert int(h[0]) == len(c) and [int(x) for x in h[1:]] == [want.get(i, 0) for i in range(1, 256)], k


@pytest.mark.parametrize("k", [1, 2, 5, 15, 16, 21, 31, 32])
def test_numpy_counter_equals_python_restatement(tmp_path, k):
    """The vectorised counter the GPU counter tests check against (a few Mbases per second) gives the pure-Python
    restatement's keys, counts and order - on reads with N, lower case, empty and short reads, repeats and palindromes,
    in one chunk and in many - and so do its histogram, its A-minus-B list and its list-file reader."""
    import numpy as np

    from oracle import unique_oracle as uo

    rng = np.random.default_rng(40 + k)
    g = "".join("ACGT"[c] for c in rng.integers(0, 4, 2500))
    comp = str.maketrans("ACGT", "TGCA")

    def lib(n):
        reads = []
        for p in rng.integers(0, 2300, n):
            r = g[p:p + int(rng.integers(0, 200))]
            if rng.random() < 0.5:
                r = r.translate(comp)[::-1]
            if rng.random() < 0.2:
                r = r.lower()
            if r and rng.random() < 0.3:
                q = int(rng.integers(0, len(r)))
                r = r[:q] + "Nn-*"[int(rng.integers(0, 4))] + r[q + 1:]
            reads.append(r)
        return reads + ["", "N", "A" * 300, "AC" * 150, "ACGT" * 80, "AAT" * 90, "acgt" * 10 + "N" + "ACGT" * 10, g[:k], g[:max(k - 1, 0)],
                        "N" + g[:k], g[:k] + "N", "", g[5:5 + k].lower()]

    reads_a, reads_b = lib(300), lib(150)
    want_a, want_b = uo.count_kmers(reads_a, k), uo.count_kmers(reads_b, k)
    for chunk in (1 << 23, 997):
        keys, counts = uo.count_kmers_np(*uo.pack(reads_a), k, chunk=chunk)
        assert keys.dtype == np.uint64 and (keys[1:] > keys[:-1]).all()
        names = uo.kmer_strings(keys, k)
        assert names == sorted(want_a) and [int(c) for c in counts] == [want_a[n] for n in names]
    a, b = (keys, counts), uo.count_kmers_np(*uo.pack(reads_b), k)
    halves = uo.add_counts_np(uo.count_kmers_np(*uo.pack(reads_a[:100]), k), uo.count_kmers_np(*uo.pack(reads_a[100:]), k))
    assert np.array_equal(halves[0], keys) and np.array_equal(halves[1], counts)
    dba, dbb = uo.database(want_a), uo.database(want_b)
    hist = uo.histogram_np(counts)
    assert int(hist[0]) == len(want_a) and int(hist[1]) == sum(1 for n in want_a.values() if n == 1)
    assert [(c, int(hist[c])) for c in range(2, 256)] == uo.histogram_rows(dba)[1:]
    assert len(dba) > 0
    for lo, hi in ((2, 255), (1, 4), (3, 9), (255, 255), (0, 1000), (5, 3)):
        got = uo.unique_np(a, b, lo, hi)
        assert uo.kmer_strings(got, k) == uo.unique_kmers(dba, dbb, lo, hi), (lo, hi)
    path = tmp_path / "list.txt"
    path.write_text("".join(n + "\n" for n in names))
    assert np.array_equal(uo.read_list_np(str(path), k), keys)
    path.write_text("".join(n + "\n" for n in names)[:-2] + "\n")
    with pytest.raises(AssertionError):
        uo.read_list_np(str(path), k)


def test_cli_arguments_mirror_the_reference(built):
    from trio_binning_amd import find_unique_kmers as fu

    a = fu.parse_args(["-k", "21", "-p", "8", "-o", "out", "-s", "tmp", "m1.fq,m2.fq.gz", "f.fq"])
    assert (a.kmer_size, a.threads, a.outpath, a.scratch_dir, a.path_to_kmc) == (21, 8, "out", "tmp", "kmc")
    assert a.read_files == ["m1.fq,m2.fq.gz", "f.fq"]
    with pytest.raises(SystemExit):
        fu.parse_args(["m.fq", "f.fq"])  # -k is required, as in the reference
