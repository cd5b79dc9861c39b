"""Drop-in boundary audited against the reference: tools/audit_against_reference.py compares configuration fields read,
preset defaults, state_dict layouts and the checkpoint plumbing (remap / update / clean_state_dict) with the reference's,
as recorded from the real reference tree in tests/golden/reference_boundary.json (`--reference DIR --write FILE`)."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_boundary_matches_reference_tree():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, os.path.join(REPO, 'tools', 'audit_against_reference.py'), '--fixture',
                        os.path.join(REPO, 'tests', 'golden', 'reference_boundary.json')], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert '0 problem(s)' in r.stdout
