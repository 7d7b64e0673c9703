cd $GRAFT_REPO_ROOT
mkdir -p tools/_build
python -c "from xpoly_amd import build; build.build(extra=['-w', '-DXPG_TRACE', '-DXPG_ANY_INLINE=__noinline__'], out='tools/_build/libxpoly_trace.so', obj='tools/_build/obj_trace')" || exit 1
echo "=== LDS kernel"; XPG_SO_PATH=$PWD/tools/_build/libxpoly_trace.so python tools/lab/probe_case_f64.py 2>&1 | grep -E "lds|hbm|six" | head -40
echo "=== HBM path"; XPG_FORCE_DEVICE_LP=1 XPG_SO_PATH=$PWD/tools/_build/libxpoly_trace.so python tools/lab/probe_case_f64.py 2>&1 | grep -E "lds|hbm|six" | head -40
