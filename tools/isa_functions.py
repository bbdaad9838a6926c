"""Split a hipcc `-S` device assembly file into its functions and print, per function whose name contains one of the filters, the
instruction text (labels, directives that carry no code and comments dropped).  Two builds' outputs can then be compared with diff."""
import re
import sys

text = open(sys.argv[1]).read()
filters = sys.argv[2:]
for m in re.finditer(r"^(\S+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
    name, body = m.group(1), m.group(2)
    if filters and not any(f in name for f in filters):
        continue
    print("==", name)
    for line in body.splitlines():
        line = line.split(";")[0].rstrip()
        if line and not line.lstrip().startswith("."):
            print(line)
