cd $GRAFT_REPO_ROOT
mkdir -p tools/_build gpurun_out
python -c "from xpoly_amd import build; build.build(extra=['-w', '-DXPG_LIFE', '-DXPG_ANY_INLINE=__noinline__'], out='tools/_build/libxpoly_life.so', obj='tools/_build/obj_life')"
XPG_SO_PATH=$PWD/tools/_build/libxpoly_life.so PYTHONPATH=$PWD python tools/lab/probe_batch_life.py ${1:-1} ${2:-768} ${3:-} 2>&1 | tee gpurun_out/batch_life.log
