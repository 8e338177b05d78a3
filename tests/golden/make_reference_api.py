"""tests/golden/reference_api.json: the names the Julia package DeepStructuredMixtures.jl defines in its src/*.jl, as an index
(no source text): every top-level function, struct, abstract type and const; the positional arities of each function's
methods; the field names of its structs; and whether the few third-party names the binding relies on occur.
test_julia_binding_names_exist_in_the_reference checks julia/DSMGPHip.jl against it, so that the check needs no copy of the
reference.  The patterns are the ones that test applied to the sources directly.

    python tests/golden/make_reference_api.py <checkout of DeepStructuredMixtures.jl>
"""
import glob
import json
import os
import re
import sys

NAME = r"(?:[^\W\d]|[∇∂])[\w!∇∂²]*"          # any Julia name the sources define (Unicode letters included)
FIELD = r"[A-Za-z_∇∂ℓσϵμ][\w!∇∂ℓσϵμ²]*"        # struct fields: the identifier pattern the test applies to the binding


def split_top(text):
    """Split at top-level commas (parentheses, brackets and braces balanced)."""
    out, depth, cur = [], 0, ""
    for ch in text:
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur.strip())
    return out


def positional_arity(sig):
    return len([a for a in split_top(sig.split(";")[0]) if a])


def index(ref):
    defined = set()
    for pat in (rf"(?m)^\s*(?:@inline\s+)?function\s+(?:\w+\.)?({NAME})\s*[({{]",
                rf"(?m)^\s*(?:@inline\s+)?(?:\w+\.)?({NAME})\([^)\n]*\)\s*(?:where[^=\n]*)?=",
                rf"(?m)^\s*(?:mutable\s+)?struct\s+({NAME})\b", rf"(?m)^\s*abstract\s+type\s+({NAME})\b",
                rf"(?m)^\s*const\s+({NAME})\b"):
        defined |= set(re.findall(pat, ref))
    arities = {}
    for m in re.finditer(rf"(?m)^\s*(?:@inline\s+)?function\s+(?:\w+\.)?({NAME})\s*\(", ref):
        i = m.end()
        depth, j = 1, i
        while depth:
            depth += ref[j] == "("
            depth -= ref[j] == ")"
            j += 1
        arities.setdefault(m.group(1), set()).add(positional_arity(ref[i:j - 1]))
    for m in re.finditer(rf"(?m)^\s*(?:@inline\s+)?(?:\w+\.)?({NAME})\(([^)\n]*)\)\s*(?:where[^=\n]*)?=", ref):
        arities.setdefault(m.group(1), set()).add(positional_arity(m.group(2)))
    fields = set()
    for m in re.finditer(r"(?ms)^\s*(?:mutable\s+)?struct\s+[^\n]*\n(.*?)^\s*end", ref):
        for line in m.group(1).splitlines():
            mm = re.match(rf"\s*({FIELD})\s*(?:::|$)", line)
            if mm:
                fields.add(mm.group(1))
    mentions = {"BiDict": r"BiDict", "children(": r"\bchildren\(", "logweights": r"\blogweights\b", ".value": r"\.value\b"}
    return {"defined": sorted(defined), "arities": {k: sorted(v) for k, v in sorted(arities.items())},
            "struct_fields": sorted(fields), "mentions": {k: bool(re.search(p, ref)) for k, p in mentions.items()}}


if __name__ == "__main__":
    files = sorted(glob.glob(os.path.join(sys.argv[1], "src", "*.jl")))
    assert files, f"no src/*.jl under {sys.argv[1]}"
    ref = "\n".join(open(f, encoding="utf-8").read() for f in files)
    out = dict(source=f"src/*.jl of DeepStructuredMixtures.jl ({len(files)} files)", **index(ref))
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_api.json"), "w", encoding="utf-8") as f:
        json.dump(out, f, indent=0, ensure_ascii=False)
        f.write("\n")
    print(len(out["defined"]), "names,", len(out["arities"]), "functions,", len(out["struct_fields"]), "struct fields")
