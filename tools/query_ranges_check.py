#!/usr/bin/env python3
"""The ray queries' address checks (csrc/query_ranges.h) under the host sanitizers: tools/query_ranges_main.cpp built with
-fsanitize=address,undefined as a program of its own and fed the table of tests/test_query_ranges.py.  CPU only, no device, nothing
loaded into Python.  Exit status 0: every case answered as the table expects and the sanitizers reported nothing."""
import importlib.util
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    spec = importlib.util.spec_from_file_location("test_query_ranges", os.path.join(ROOT, "tests", "test_query_ranges.py"))
    table = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(table)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "query_ranges")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-fno-omit-frame-pointer", os.path.join(ROOT, "tools", "query_ranges_main.cpp"), "-o", exe])
        text = "".join("%d %d %s\n" % (n, len(bases), " ".join(map(str, bases + strides + aligns))) for _, n, bases, strides, aligns, _, _ in table.CASES)
        run = subprocess.run([exe], input=text, capture_output=True, text=True)
    sys.stderr.write(run.stderr)
    answers = run.stdout.splitlines()
    bad = 0 if run.returncode == 0 and not run.stderr and len(answers) == len(table.CASES) else 1
    for (label, _, _, _, _, code, words), answer in zip(table.CASES, answers):
        if int(answer.split()[0]) != code or not all(w in answer for w in words):
            print("MISMATCH %s: expected %d %s, got %s" % (label, code, words, answer))
            bad = 1
    print("query_ranges_check: %d cases, exit status %d, %s" % (len(table.CASES), run.returncode, "clean" if not bad else "FAILED"))
    return bad


if __name__ == "__main__":
    sys.exit(main())
