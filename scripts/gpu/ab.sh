# A/B on one box: library builds (scripts/ab/*.so)
O=gpurun_out/${1:-ab}; mkdir -p $O
timeout 1500 bash scripts/ab_bench.sh $O scripts/ab/libdynogfx_cur.so scripts/ab/libdynogfx_w4.so scripts/ab/libdynogfx_swz0.so
