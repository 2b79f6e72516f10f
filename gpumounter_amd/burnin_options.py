"""The burn-in's command line, declared once: the five ``--burn-in*`` options of ``probe``,
``doctor`` and ``parallel.validate`` and the rule for how they go together. The values are parsed
by ``ops.probe`` and ``ops.mxgemm``, which are imported only when an option is given."""
from __future__ import annotations

import argparse


def _parsed_by(module: str, name: str):
    """An argparse type from a parser in ``gpumounter_amd.ops``: its refusal a usage error."""
    def conv(text):
        from importlib import import_module

        from gpumounter_amd.ops.probe import ProbeError
        try:
            return getattr(import_module(f"gpumounter_amd.ops.{module}"), name)(text)
        except ProbeError as e:
            raise argparse.ArgumentTypeError(str(e)) from None
    conv.__name__ = name
    return conv


def add_options(p, what: str) -> None:
    """Declares the options on ``p`` (``what``: the tool's words for ``--burn-in`` itself)."""
    p.add_argument("--burn-in", type=float, default=0.0, metavar="SECONDS", help=what)
    p.add_argument("--burn-in-flip", type=_parsed_by("probe", "parse_burn_in_flip"),
                   action="append", default=None, metavar="ELEM:MASK",
                   help="with --burn-in: negative control (repeatable), for every chosen format: "
                        "XOR that bf16 element of the burn-in's reference result with MASK; the "
                        "burn-in must fail")
    p.add_argument("--burn-in-format", type=_parsed_by("mxgemm", "parse_burn_in_formats"),
                   default=None, metavar="LIST",
                   help="with --burn-in: the burn-in's formats, of bf16,mxfp8,mxfp4 (default "
                        "bf16); each runs for SECONDS, the block-scaled ones as a bit-checked "
                        "fp8 / fp4 GEMM on the MX matrix pipe")
    p.add_argument("--burn-in-attribute", action="store_true",
                   help="with --burn-in: rotate the GEMM's tiles over the blocks from one "
                        "iteration to the next, so other XCDs and CUs recompute every tile, "
                        "record the CU of every block and name the units behind a mismatch")
    p.add_argument("--burn-in-inject", type=_parsed_by("probe", "parse_burn_in_inject"),
                   default=None, metavar="ID|first:MASK",
                   help="with --burn-in-attribute: negative control: every block on that CU "
                        "(first: the one that computed tile 0 in the warm-up) XORs MASK into "
                        "one element of its tile, in the reference too; the burn-in must fail "
                        "and name that unit alone")


def usage(args, format_first: bool = True, name_pair: bool = False) -> str:
    """What is wrong with the options as parsed, or "". Each tool keeps the words it has always
    used: ``probe`` looks at the flip before the format (``format_first=False``), and ``validate``
    names both options of a pair where one of them lacks ``--burn-in`` (``name_pair``)."""
    flip, fmt = "--burn-in-flip", "--burn-in-format"
    given = {flip: args.burn_in_flip, fmt: args.burn_in_format,
             "--burn-in-attribute": args.burn_in_attribute, "--burn-in-inject": args.burn_in_inject}
    pairs = ((fmt, flip) if format_first else (flip, fmt),
             ("--burn-in-attribute", "--burn-in-inject"))
    if not args.burn_in:
        for first, second in pairs:
            if name_pair and (given[first] or given[second]):
                return f"{first} and {second} need --burn-in SECONDS"
            for option in (first, second):
                if given[option]:
                    return f"{option} needs --burn-in SECONDS"
    if args.burn_in_inject and not args.burn_in_attribute:
        return "--burn-in-inject needs --burn-in-attribute"
    return ""
