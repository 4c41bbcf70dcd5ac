"""Test-only restatement of the read-level analysis of the reference's src/merge_lists.py:160-179, from dict
databases: plain Python, the reference's own arithmetic (ints that turn float at the first `+= 1/len(matches)`,
additions in window order), no numpy in the sums."""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence, Tuple

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def canonical(kmer: str) -> str:
    """:60-73; KeyError on anything but upper-case ACGT (:66)."""
    comp = ""
    for ch in kmer:
        comp += _COMP[ch]
    rev_comp = comp[::-1]
    return kmer if kmer < rev_comp else rev_comp


def read_votes(read: str, k: int, datasets: Sequence[Iterable[str]], pivot: Optional[Iterable[str]] = None
               ) -> Tuple[List[float], List[int], int]:
    """One read -> (votes, the datasets that tie for max(votes), k-mers no dataset holds).  datasets[d]: the
    canonical k-mers (strings) of dataset d — sets or dicts; pivot: the pivot dictionary, a k-mer missing from it
    raises KeyError as :167 does (None: every k-mer counts as present)."""
    n = len(datasets)
    votes = [0 for _ in range(n)]
    count = 0
    for i in range(0, len(read) - k + 1):                    # :53-58
        canon = canonical(read[i:i + k])
        if pivot is not None and canon not in pivot:
            raise KeyError(canon)
        matches = [d for d in range(n) if canon in datasets[d]]      # ascending, as update_dictionary appends
        if len(matches) > 0:
            for m in matches:
                votes[m] += 1 / len(matches)
        else:
            count += 1
    top = max(votes)                                         # ValueError for n == 0, as the reference
    ties = [d for d in range(n) if votes[d] == top]
    return votes, ties, count


def reads_votes(reads: Sequence[str], k: int, datasets, pivot=None):
    return [read_votes(r, k, datasets, pivot) for r in reads]


def tie_masks(results, num_datasets: int):
    """The ties of `reads_votes` as uint64[nreads, nwords] bit masks (the layout of Engine.read_votes)."""
    import numpy as np
    nw = max(1, (num_datasets + 63) // 64)
    out = np.zeros((len(results), nw), dtype=np.uint64)
    for r, (_, ties, _) in enumerate(results):
        for d in ties:
            out[r, d // 64] |= np.uint64(1) << np.uint64(d % 64)
    return out


def file_reads(text: str) -> List[str]:
    """The reads of a pivot_N.fa given as a str, by :153-159 (universal newlines, no '>' in the line, strip)."""
    import io
    return [line.strip() for line in io.StringIO(text, newline=None).readlines() if ">" not in line]
