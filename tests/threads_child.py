"""A process whose FIRST GPU work happens in two threads at once: one creates a pose context and runs the pose script, the other a facenet
context and the face script (context_scripts.py).  This is where the launchers' first-use flags, the first hipFuncSetAttribute of every
kernel and the empty plan caches meet two threads.  Prints one JSON line {"pose": {name: SHA-256}, "face": {...}};
tests/test_gpu_threads.py starts it once and compares the digests with its own serial reference."""
import importlib
import json
import os
import sys
import threading
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import context_scripts as CS      # noqa: E402

JOIN_SECONDS = 240


def main():
    native = importlib.import_module(CS.PKG + '.native')
    native.load()                                       # (the shared library only: no device call yet)
    out, errors = {}, []
    barrier = threading.Barrier(2)

    def pose():
        eng = native.Engine(0, **CS.POSE)
        try:
            eng.set_weights(CS.pose_weights(native))
            out['pose'] = CS.digests(CS.pose_script(eng))
        finally:
            eng.close()

    def face():
        eng = native.Engine(0, **CS.FACE)
        try:
            eng.set_weights(CS.face_weights())
            out['face'] = CS.digests(CS.face_script(eng))
        finally:
            eng.close()

    def wrap(fn):
        try:
            barrier.wait(timeout=JOIN_SECONDS)
            fn()
        except BaseException:
            errors.append(traceback.format_exc())
            barrier.abort()

    threads = [threading.Thread(target=wrap, args=(fn,), daemon=True) for fn in (pose, face)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_SECONDS)
    if any(t.is_alive() for t in threads):
        sys.stderr.write('a thread is still running after %d s\n' % JOIN_SECONDS)
        sys.stderr.flush()
        os._exit(3)
    if errors:
        sys.stderr.write('\n'.join(errors))
        return 2
    print(json.dumps(out, sort_keys=True))
    return 0


if __name__ == '__main__':
    sys.exit(main())
