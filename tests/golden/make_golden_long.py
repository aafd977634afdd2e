"""Generate the long-sequence goldens (long_cases.py) by running the REFERENCE itself: make_golden.py's stubs and its run_case,
which asserts oracle == reference before it stores anything (build container only; see make_golden.py).

    python tests/golden/make_golden_long.py [case ...]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                        # tests/helpers.py
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))       # oracle/

import make_golden  # noqa: E402
from long_cases import LONG_CASES  # noqa: E402


def main():
    make_golden.install_stubs()
    only = sys.argv[1:]
    for name, c in LONG_CASES.items():
        if not only or name in only:
            make_golden.run_case(name, c)


if __name__ == "__main__":
    main()
