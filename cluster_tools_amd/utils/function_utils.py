"""Job log protocol (cluster_tools/utils/function_utils.py:7-22).

Jobs write to stdout, which LocalTask/SlurmTask/LSFTask redirect into
tmp_folder/logs/<task>_<job>.log.  A job succeeded iff its last line is
"<datetime>: processed job <id>"; finished blocks are "<datetime>: processed block <id>".

The rest is what every job script shares: the device of the job, the read-ahead loop over its
blocks, the config preamble and the entry point.
"""
import json
import os
import sys
from concurrent import futures
from contextlib import contextmanager
from datetime import datetime
from subprocess import check_output


def log(msg):
    print("%s: %s" % (str(datetime.now()), msg), flush=True)


def log_block_success(block_id):
    print("%s: processed block %i" % (str(datetime.now()), block_id), flush=True)


def log_job_success(job_id):
    print("%s: processed job %i" % (str(datetime.now()), job_id), flush=True)


def device():
    """The GPU of this job: CTWS_DEVICE (set per job by the task), else the launcher's LOCAL_RANK."""
    return int(os.environ.get('CTWS_DEVICE', os.environ.get('LOCAL_RANK', '0')))


@contextmanager
def read_ahead(read, items):
    """Iterate (item, future of read(item)) with exactly one read running ahead of the loop body, on
    one reader thread.  read(items[0]) is submitted on entry; when the pair of item k is handed out,
    read(items[k + 1]) has been submitted and nothing later.  The body calls future.result() itself."""
    with futures.ThreadPoolExecutor(1) as io:
        first = io.submit(read, items[0]) if len(items) else None

        def pairs(ahead):
            for k, item in enumerate(items):
                cur = ahead
                ahead = io.submit(read, items[k + 1]) if k + 1 < len(items) else None
                yield item, cur
        yield pairs(first)


def load_config(job_id, config_path):
    log("start processing job %i" % job_id)
    log("reading config from %s" % config_path)
    with open(config_path) as f:
        return json.load(f)


def job_id_from_path(path):
    """<task_name>_<job_id>.config -> job_id"""
    return int(os.path.split(path)[1].split('.')[0].split('_')[-1])


def run_job(job):
    """The __main__ of a job script: `script.py <config_path>`."""
    path = sys.argv[1]
    assert os.path.exists(path), path
    job(job_id_from_path(path), path)


def chunk_id(block, blocking):
    return tuple(int(beg // ch) for beg, ch in zip(block.begin, blocking.blockShape))


def tail(path, n_lines):
    return check_output(['tail', '-%i' % n_lines, path]).decode().split('\n')[:-1]
