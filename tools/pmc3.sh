#!/bin/bash
# usage: tools/pmc3.sh <tag> <N> <frames> <tiles>
TAG=$1; N=$2; FR=$3; TL=$4
R=$GRAFT_REPO_ROOT
OUT=$(realpath -m "${OUT:-out}"); mkdir -p "$OUT"     # output directory (relative to the directory this is started from: the repository root)
cd /tmp && export TMPDIR=/tmp
i=0
for C in "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_VALU SQ_LDS_BANK_CONFLICT" \
         "SQ_ACTIVE_INST_LDS SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_ANY SQ_INSTS_SALU SQ_ACTIVE_INST_ANY SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAIT_INST_LDS" \
         "SQ_VMEM_WR_TA_DATA_FIFO_FULL SQ_VMEM_TA_ADDR_FIFO_FULL SQ_VMEM_TA_CMD_FIFO_FULL SQ_LDS_DATA_FIFO_FULL SQ_LDS_CMD_FIFO_FULL SQ_INST_LEVEL_VMEM SQ_INST_CYCLES_VMEM_WR SQ_INST_CYCLES_VMEM_RD" \
         "FETCH_SIZE" "WRITE_SIZE" "TCC_HIT_sum TCC_MISS_sum" "GRBM_GUI_ACTIVE" "TCC_EA0_WRREQ_sum TCC_EA0_WRREQ_64B_sum" "TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum" "TCP_TCC_READ_REQ_sum TCP_TCC_WRITE_REQ_sum" "TCC_REQ_sum TCC_WRITE_sum TCC_READ_sum"; do
  i=$((i+1))
  rocprofv3 --pmc $C --output-format csv -d $OUT/pmc_${TAG}/p$i -- python3 $R/tools/run_frames.py $N $FR $TL > $OUT/pmc_${TAG}_p$i.log 2>&1 || tail -3 $OUT/pmc_${TAG}_p$i.log
done
python3 $R/tools/pmc_summary.py $OUT/pmc_${TAG} | tee $OUT/pmc_${TAG}_summary.txt
