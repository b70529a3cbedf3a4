"""python tools/count_code_lines.py i2v-adapter-unofficial_amd/*.py -- per file and in total, the lines that hold code: not blank, not a
comment, not part of a docstring.  The size figure of a refactor."""
import ast
import sys
import tokenize

SKIP = (tokenize.COMMENT, tokenize.NL, tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT, tokenize.ENDMARKER)


def code_lines(path):
    doc = set()
    for n in ast.walk(ast.parse(open(path).read())):
        b = getattr(n, "body", None)
        if isinstance(n, (ast.Module, ast.ClassDef, ast.FunctionDef)) and b and isinstance(b[0], ast.Expr) \
                and isinstance(b[0].value, ast.Constant) and isinstance(b[0].value.value, str):
            doc.update(range(b[0].lineno, b[0].end_lineno + 1))
    with open(path) as f:
        code = {l for t in tokenize.generate_tokens(f.readline) if t.type not in SKIP for l in range(t.start[0], t.end[0] + 1)}
    return len(code - doc)


if __name__ == "__main__":
    counts = [(code_lines(p), p) for p in sys.argv[1:]]
    for n, p in counts:
        print(n, p)
    print(sum(n for n, _ in counts), "total")
