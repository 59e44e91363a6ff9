"""Loads a build of the library in a child process and checks that it exports every entry of the Python binding (_lib.SIGNATURES, _lib.QUERIES):
what _lib.load() will look up.  usage: python scripts/check_lib_symbols.py path/to/lib.so"""
import os
import subprocess
import sys

CHILD = '''
import ctypes, importlib.util, sys
spec = importlib.util.spec_from_file_location('_y2lib', sys.argv[2])
m = importlib.util.module_from_spec(spec)
spec.loader.exec_module(m)
lib = ctypes.CDLL(sys.argv[1])
missing = [n for n in list(m.SIGNATURES) + list(m.QUERIES) if not hasattr(lib, n)]
if missing:
    sys.exit('%s lacks %d symbols: %s' % (sys.argv[1], len(missing), ' '.join(missing)))
print('%s: all %d symbols present' % (sys.argv[1], len(m.SIGNATURES) + len(m.QUERIES)))
'''

if __name__ == '__main__':
    lib_py = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'yolo_tf_amd', '_lib.py')
    sys.exit(subprocess.call([sys.executable, '-c', CHILD, os.path.abspath(sys.argv[1]), lib_py]))
