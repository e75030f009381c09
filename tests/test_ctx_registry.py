"""CPU test of the registry behind every C ABI handle (deep-active-inference-mc_amd/csrc/ctx_registry.h): tests/ctx_registry_check.cpp
drives it on a fake context with a counting deleter, built with g++ under ThreadSanitizer.  efe_destroy racing calls in flight is tested
here and not on the GPU, where a wrong answer would free buffers under running kernels."""
import os
import subprocess

from conftest import ROOT

CHECKS = [
    'unknown: nullptr is refused',
    'unknown: a made-up pointer is refused',
    'unknown: an object that was never inserted is refused',
    'unknown: retiring an unknown handle deletes nothing',
    'holder: an inserted context is alive',
    'holder: retirement did not return while an admitted call held the lock',
    'holder: the deleter ran once, after the holder let go',
    'holder: a retired handle is refused',
    'holder: a second retirement is a no-op',
    'dead: a context marked dead is refused',
    'dead: retiring it runs the deleter once',
    'concurrent: admissions succeed while the context is live',
    'concurrent: no admission succeeds after retirement returns',
    'concurrent: a retired context is not alive',
    'concurrent: the deleter ran exactly once',
    'concurrent: the deleter ran after the last holder was gone',
]


def test_registry_admission_and_retirement_under_tsan(tmp_path):
    exe = str(tmp_path / 'ctx_registry_check')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-pthread', '-fsanitize=thread', '-Wall', '-Werror',
           '-I', os.path.join(ROOT, 'deep-active-inference-mc_amd', 'csrc'), os.path.join(ROOT, 'tests', 'ctx_registry_check.cpp'), '-o', exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    env = dict(os.environ, TSAN_OPTIONS='halt_on_error=1 exitcode=66')
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert 'ThreadSanitizer' not in r.stderr, r.stderr
    assert r.returncode == 0, r.stdout + r.stderr
    passed = {line[3:] for line in r.stdout.splitlines() if line.startswith('ok ')}
    assert passed == set(CHECKS), sorted(set(CHECKS) ^ passed)
    assert r.stdout.rstrip().endswith('ALL OK')
