"""CPU-only: how many compile processes constriction_amd.build starts (MAX_JOBS, the CPU count, the number of sources)."""
import os

import pytest

from constriction_amd import build


@pytest.mark.parametrize("max_jobs, n_sources, want", [
    (None, 1000, os.cpu_count() or 1),      # unset: every CPU
    ("16", 1000, 16),
    ("16", 5, 5),                           # never more workers than sources
    ("0", 1000, os.cpu_count() or 1),       # not a count: as if unset
    ("abc", 1000, os.cpu_count() or 1),
    ("", 1000, os.cpu_count() or 1),
    ("3", 0, 1),                            # and never fewer than one
])
def test_workers(monkeypatch, max_jobs, n_sources, want):
    if max_jobs is None:
        monkeypatch.delenv("MAX_JOBS", raising=False)
    else:
        monkeypatch.setenv("MAX_JOBS", max_jobs)
    assert build._workers(n_sources) == want
