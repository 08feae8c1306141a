#!/usr/bin/env python
"""Records tests/golden/gram_tail_bits_parent.json (or the path given): one SHA-256 per case of tests/test_gpu_gram_tail_bits.py
over the raw output bytes of the cost paths.  Needs an MI355X; run on the commit whose bits are to be the yardstick (see that
module's docstring for when that is), or against a build of it through KCCOT_LIB_PATH: the C ABI is that commit's."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_gpu_gram_tail_bits as tb    # noqa: E402

if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else tb.GOLDEN
    res = {name: tb.case(name) for name in tb.CASES}
    with open(path, "w") as f:
        f.write('{"sha256": {\n' + ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(res[k])) for k in sorted(res)) + "\n}}\n")
    print("wrote %s (%d cases)" % (path, len(res)))
