"""Argument checks that the atomics and the host-sync test share (``ops.atomics``,
``ops.hostsync``): an integer in a range, a power of two, and a test given by name or by bit, a
set of them, a comma-separated list of them. Each module binds one :class:`Checks` with its label
(the word its messages start with) and its ``TESTS`` table."""
from __future__ import annotations

from typing import Dict, Iterable, Tuple

from gpumounter_amd.ops.probe import ProbeError


class Checks:
    def __init__(self, label: str, tests: Dict[str, int]):
        self.label, self.tests = label, tests
        self.names = {v: k for k, v in tests.items()}

    def int_in(self, v, lo: int, hi: int, what: str) -> int:
        if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
            raise ProbeError(f"{self.label}: {what} must be an integer in [{lo}, {hi}], got {v!r}")
        return v

    def pow2(self, v, hi: int, what: str) -> int:
        self.int_in(v, 1, hi, what)
        if v & (v - 1):
            raise ProbeError(f"{self.label}: {what} must be a power of two, got {v}")
        return v

    def bit_of(self, test) -> int:
        """The bit of one test, given by name or by bit."""
        if isinstance(test, str) and test in self.tests:
            return self.tests[test]
        if isinstance(test, int) and not isinstance(test, bool) and test in self.names:
            return test
        raise ProbeError(f"unknown {self.label} test {test!r} (one of {', '.join(self.tests)})")

    def mask_of(self, tests: Iterable) -> int:
        if isinstance(tests, (str, int)):
            tests = (tests,)
        mask = 0
        for t in tests:
            mask |= self.bit_of(t)
        if not mask:
            raise ProbeError(f"{self.label} needs at least one test")
        return mask

    def parse_tests(self, text) -> Tuple[str, ...]:
        """``"add,ticket,cas"`` → ("add", "ticket", "cas"); every name is checked."""
        names = tuple(t.strip() for t in str(text).split(",") if t.strip())
        self.mask_of(names)
        return names
